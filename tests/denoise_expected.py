"""The denoiser's contract (include/rt_hip.h, rt_hip_denoise) restated in numpy: vectorised over the pixels, sequential over the 25
taps in the contract's order, fp64 +, -, *, / in the written order (numpy's float64 arithmetic is IEEE and never fuses), every
stored intermediate rounded to float32.  A skipped tap is not added (np.where keeps the old sum)."""
import numpy as np

EPS = 2.0 ** -10
H5 = (1.0 / 16, 1.0 / 4, 3.0 / 8, 1.0 / 4, 1.0 / 16)
DEMODULATE, OBJECT_EDGES = 1, 2
DEFAULTS = dict(iterations=5, sigma_color=0.5, normal_power_log2=3, sigma_depth=1.0, flags=DEMODULATE)


def denoise(rgb, albedo, normal, depth, hits, obj, iterations=5, sigma_color=0.5, normal_power_log2=3, sigma_depth=1.0,
            flags=DEMODULATE):
    """rgb, albedo, normal: float32 [H,W,3]; depth float32 [H,W]; hits, obj uint32 [H,W] (albedo / obj may be None when the flags
    do not need them) -> the denoised float32 [H,W,3]"""
    c = np.asarray(rgb, np.float32)
    h, w = c.shape[:2]
    valid = np.isfinite(c).all(axis=2)
    demod = bool(flags & DEMODULATE)
    edges = bool(flags & OBJECT_EDGES)
    with np.errstate(all="ignore"):
        a = np.asarray(albedo, np.float32).astype(np.float64) + EPS if demod else None
        e = (c.astype(np.float64) / a).astype(np.float32) if demod else c.copy()
        n = np.asarray(normal, np.float32).astype(np.float64)
        z = np.asarray(depth, np.float32).astype(np.float64)
        hit = np.asarray(hits, np.uint32)
        o = np.asarray(obj, np.uint32) if edges else None
        ys, xs = np.mgrid[0:h, 0:w]
        for i in range(iterations):
            s = 1 << i
            sigma = sigma_color * 2.0 ** -i
            S2 = sigma * sigma
            ep = e.astype(np.float64)
            W = np.zeros((h, w))
            A = np.zeros((h, w, 3))
            Dp = sigma_depth * z
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    if dx == 0 and dy == 0:
                        wc = 9.0 / 64.0
                        W = W + wc
                        A = A + wc * ep
                        continue
                    qx, qy = xs + s * dx, ys + s * dy
                    inside = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                    qxc, qyc = np.where(inside, qx, xs), np.where(inside, qy, ys)
                    eq = ep[qyc, qxc]
                    take = inside & valid[qyc, qxc]
                    if edges:
                        take &= o[qyc, qxc] == o
                    bg_p, bg_q = hit == 0, hit[qyc, qxc] == 0
                    take &= bg_p == bg_q
                    nq = n[qyc, qxc]
                    g = (n[..., 0] * nq[..., 0] + n[..., 1] * nq[..., 1]) + n[..., 2] * nq[..., 2]
                    g = np.where(g > 0, g, 0.0)
                    wn = g
                    for _ in range(normal_power_log2):
                        wn = wn * wn
                    D = Dp * float(s * max(abs(dx), abs(dy)))
                    Zn = D * D
                    dz = z[qyc, qxc] - z
                    Zd = Zn + dz * dz
                    zero = Zd == 0
                    Zn, Zd = np.where(zero, 1.0, Zn), np.where(zero, 1.0, Zd)
                    both = bg_p & bg_q
                    wn, Zn, Zd = np.where(both, 1.0, wn), np.where(both, 1.0, Zn), np.where(both, 1.0, Zd)
                    de = eq - ep
                    dc = (de[..., 0] * de[..., 0] + de[..., 1] * de[..., 1]) + de[..., 2] * de[..., 2]
                    wt = (((H5[dx + 2] * H5[dy + 2]) * wn) * (S2 * Zn)) / ((S2 + dc) * Zd)
                    W = np.where(take, W + wt, W)
                    A = np.where(take[..., None], A + wt[..., None] * eq, A)
            e = np.where(valid[..., None], (A / W[..., None]).astype(np.float32), e)
        out = (e.astype(np.float64) * a).astype(np.float32) if demod else e.copy()
    return np.where(valid[..., None], out, c)


def denoise_aov(rgb, aov, **params):
    """denoise() with the buffers in a dict as GpuScene.aov_image gives them"""
    return denoise(rgb, aov.get("albedo"), aov["normal"], aov["depth"], aov["hits"], aov.get("object"), **params)


def same_floats(got, exp):
    """bit for bit, NaN equal to NaN (any payload)"""
    g, e = np.asarray(got, np.float32), np.asarray(exp, np.float32)
    both_nan = np.isnan(g) & np.isnan(e)
    return bool(((g.view(np.uint32) == e.view(np.uint32)) | both_nan).all())


FLT_MAX = float(np.finfo(np.float32).max)
DENORM_MIN, DENORM_MAX = 2.0 ** -149, 2.0 ** -126 - 2.0 ** -149   # the smallest and the largest float32 denormal
# what _edge_inputs plants.  COLD values keep a valid pixel finite at the default parameters (most of them); a HOT value makes a
# valid pixel's signal inf or NaN -- albedo -2^-10 divides by zero, FLT_MAX over an albedo below 1 overflows the float,
# sigma_depth * (+-inf) gives Zn / Zd = inf / inf -- and a non-finite signal reaches every pixel that takes it as a tap (w * e_q
# with w = 0 is NaN as well): within 62 pixels after five iterations.
COLD = ("flt_max", "neg_flt_max", "denormal", "neg_zero", "negative", "albedo_zero", "albedo_denormal", "albedo_flt_max",
        "albedo_negative", "depth_flt_max", "depth_denormal", "depth_negative", "depth_zero_run", "normal_zero", "normal_1e19",
        "normal_1e-19", "miss_with_depth", "no_object_id", "invalid")
HOT = ("albedo_minus_eps", "flt_max_overflow", "depth_minus_inf", "hit_with_inf_depth")


def _edge_inputs(w, h, rng, hot_band=0.125, share=0.4):
    """buffers of ordinary values (colours in [0, 30], albedo in [0.05, 1], unit normals, depths in [1, 21], 1..3 hits, a tenth
    ordinary background) with the values of COLD and HOT planted: pixels taken in a random order, `share` of them planted
    (2 of every 5 at the default), the categories in turn -- so each category holds share / (len(COLD) + len(HOT)) of the
    pixels, up to rounding, and every planted pixel has ordinary pixels among its taps.  A pixel that draws a HOT category at
    x >= hot_band * w stays ordinary: the hot values, whose damage spreads, live in the left band only (hot_band = 0: none,
    1: everywhere).  -> rgb, dict of the first-hit buffers, planted: category -> pixel indices y * w + x"""
    n = w * h
    rgb = (rng.random((h, w, 3)) * rng.choice([0.1, 1.0, 30.0], (h, w, 1))).astype(np.float32)
    albedo = (0.05 + 0.95 * rng.random((h, w, 3))).astype(np.float32)
    nn = rng.normal(size=(h, w, 3))
    normal = (nn / np.linalg.norm(nn, axis=2, keepdims=True)).astype(np.float32)
    depth = (1.0 + 20.0 * rng.random((h, w))).astype(np.float32)
    hits = rng.integers(1, 4, (h, w)).astype(np.uint32)
    obj = rng.integers(0, 3, (h, w)).astype(np.uint32)
    bg = rng.random((h, w)) < 0.1
    hits[bg], obj[bg], depth[bg], normal[bg] = 0, 0xFFFFFFFF, np.inf, 0
    rgb[bg] = np.float32(10 / 255)
    cats = COLD + HOT
    planted = {c: [] for c in cats}
    order = rng.permutation(n)
    per5 = int(round(share * 5))
    drawn = np.zeros(n, bool)
    drawn[order[np.arange(n) % 5 < per5]] = True
    k = 0
    for i, p in enumerate(order):
        if i % 5 >= per5:
            continue
        cat = cats[k % len(cats)]
        k += 1
        y, x = divmod(int(p), w)
        if cat in HOT and not x < hot_band * w:
            continue
        planted[cat].append(int(p))
        if bg[y, x] and cat not in ("miss_with_depth", "invalid"):   # the value goes on a hit pixel
            hits[y, x], obj[y, x], depth[y, x], normal[y, x] = 2, 1, np.float32(7.5), np.float32([0.6, 0.0, 0.8])
        if cat == "flt_max":
            rgb[y, x], albedo[y, x] = FLT_MAX, 1.0
        elif cat == "neg_flt_max":
            rgb[y, x, int(rng.integers(0, 3))], albedo[y, x] = -FLT_MAX, 1.0
        elif cat == "denormal":
            rgb[y, x] = [DENORM_MIN, DENORM_MAX, 3 * DENORM_MIN]
        elif cat == "neg_zero":
            rgb[y, x] = -0.0
        elif cat == "negative":
            rgb[y, x] = -rgb[y, x] - np.float32(0.25)
        elif cat == "albedo_zero":
            albedo[y, x] = 0
        elif cat == "albedo_denormal":
            albedo[y, x] = [DENORM_MIN, DENORM_MAX, 0.5]
        elif cat == "albedo_flt_max":
            albedo[y, x] = FLT_MAX
        elif cat == "albedo_negative":
            albedo[y, x] = -albedo[y, x]
        elif cat == "depth_flt_max":
            depth[y, x] = FLT_MAX
        elif cat == "depth_denormal":
            depth[y, x] = DENORM_MIN * int(rng.integers(1, 100))
        elif cat == "depth_negative":
            depth[y, x] = -depth[y, x]
        elif cat == "depth_zero_run":   # up to three hit pixels in a row at depth 0 (no other drawn pixel): D = dz = 0, so Zd == 0
            for xx in range(x, min(x + 3, w)):
                if xx > x and drawn[y * w + xx]:
                    break
                depth[y, xx] = 0
                if hits[y, xx] == 0:
                    hits[y, xx], obj[y, xx], normal[y, xx] = 1, 1, np.float32([0.0, 0.0, 1.0])
        elif cat == "normal_zero":
            normal[y, x] = 0
        elif cat == "normal_1e19":
            normal[y, x] = normal[y, x] * np.float32(1e19)
        elif cat == "normal_1e-19":
            normal[y, x] = normal[y, x] * np.float32(1e-19)
        elif cat == "miss_with_depth":
            hits[y, x], depth[y, x] = 0, np.float32(3.25)
        elif cat == "no_object_id":
            obj[y, x] = 0xFFFFFFFF
        elif cat == "invalid":
            rgb[y, x, int(rng.integers(0, 3))] = [np.nan, np.inf, -np.inf][int(rng.integers(0, 3))]
        elif cat == "albedo_minus_eps":
            albedo[y, x] = [-EPS, -EPS, 0.5]
        elif cat == "flt_max_overflow":
            rgb[y, x] = [FLT_MAX, -FLT_MAX, 1.0]
            albedo[y, x] = 0.5
        elif cat == "depth_minus_inf":
            depth[y, x] = -np.inf
        elif cat == "hit_with_inf_depth":
            depth[y, x] = np.inf
    return rgb, dict(albedo=albedo, normal=normal, depth=depth, hits=hits, object=obj), {c: np.array(v, int) for c, v in planted.items()}

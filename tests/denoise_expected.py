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

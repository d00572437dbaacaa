"""The probe visibility of include/rt_hip.h ("probe visibility") restated on the CPU, twice: one numpy form, vectorised, and one plain
scalar Python form of the same text, one double at a time.  Python floats and numpy float64 are IEEE doubles, + - * / and sqrt
correctly rounded and never fused: what the contract asks of the device.  The octahedral map, the depth fold, the resolve and the
extended shade; the grid's cells and the SH9 evaluation are tests/probe_grid_expected.py's and tests/probe_expected.py's.
"""
import math

import numpy as np

from probe_expected import A, QNAN, sh_bases, sh_basis_scalar
from probe_grid_expected import FACE_FLOOR, FACING, INV_PI, _cells


class Vis:
    """an RtHipProbeVis' fields; the defaults are rt_hip_probe_vis_defaults' for a grid of the given step"""

    def __init__(self, step=(1.0, 1.0, 1.0), res=8, sharp=5, d_max=None, bias=None, floor=2.0 ** -6):
        sx, sy, sz = (float(x) for x in step)
        self.res, self.sharp = int(res), int(sharp)
        self.d_max = 1.5 * math.sqrt((sx * sx + sy * sy) + sz * sz) if d_max is None else float(d_max)
        self.bias = 0.125 * min(sx, sy, sz) if bias is None else float(bias)
        self.floor = float(floor)

    def abi(self, grid=None):
        from rt_amd import abi
        return abi.probe_vis(grid, self.res, self.sharp, self.d_max, self.bias, self.floor)


# ---- the map ------------------------------------------------------------------------------------------------------------------------------
def _sgn(v):
    return np.where(v >= 0.0, 1.0, -1.0)


def texel_dirs(R):
    """-> float64 [R*R, 3]: the centre direction of texel tx + R*ty"""
    i = np.arange(R * R)
    tx, ty = (i % R).astype(np.float64), (i // R).astype(np.float64)
    a = ((tx + 0.5) / float(R)) * 2.0 - 1.0
    b = ((ty + 0.5) / float(R)) * 2.0 - 1.0
    z = (1.0 - np.abs(a)) - np.abs(b)
    x = np.where(z < 0.0, (1.0 - np.abs(b)) * _sgn(a), a)
    y = np.where(z < 0.0, (1.0 - np.abs(a)) * _sgn(b), b)
    k = 1.0 / np.sqrt((x * x + y * y) + z * z)
    return np.stack([x * k, y * k, z * k], axis=1)


def texel_dir_scalar(R, tx, ty):
    a = ((float(tx) + 0.5) / float(R)) * 2.0 - 1.0
    b = ((float(ty) + 0.5) / float(R)) * 2.0 - 1.0
    z = (1.0 - abs(a)) - abs(b)
    x, y = a, b
    if z < 0.0:
        x = (1.0 - abs(b)) * (1.0 if a >= 0.0 else -1.0)
        y = (1.0 - abs(a)) * (1.0 if b >= 0.0 else -1.0)
    k = 1.0 / math.sqrt((x * x + y * y) + z * z)
    return (x * k, y * k, z * k)


def sample_position(R, v):
    """steps 1 and 2 of the lookup -> (ux, uy) float64 [m]: the sample position in texels, clamped to [-0.5, R - 0.5]"""
    v = np.asarray(v, dtype=np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        s = (np.abs(v[:, 0]) + np.abs(v[:, 1])) + np.abs(v[:, 2])
        a, b = v[:, 0] / s, v[:, 1] / s
        fa, fb = (1.0 - np.abs(b)) * _sgn(a), (1.0 - np.abs(a)) * _sgn(b)
        a, b = np.where(v[:, 2] < 0.0, fa, a), np.where(v[:, 2] < 0.0, fb, b)
        out = []
        for c in (a, b):
            u = (c * 0.5 + 0.5) * float(R) - 0.5
            u = np.where(u >= -0.5, u, -0.5)
            top = float(R) - 0.5
            out.append(np.where(u <= top, u, top))
    return out[0], out[1]


def _texel(R, i, j):
    """step 3: (i, j) continued across the map's edge -> the texel's index"""
    out = (i < 0) | (i > R - 1)
    i2 = np.where(out, np.where(i < 0, 0, R - 1), i)
    j2 = np.where(out, R - 1 - j, j)
    out = (j2 < 0) | (j2 > R - 1)
    j3 = np.where(out, np.where(j2 < 0, 0, R - 1), j2)
    i3 = np.where(out, R - 1 - i2, i2)
    return i3 + R * j3


def lookup(moments, probe, R, v):
    """moments [N, R*R, 2], probe int [m], v [m, 3] -> (mean, mean2) float64 [m]"""
    ux, uy = sample_position(R, v)
    fl_x, fl_y = np.floor(ux), np.floor(uy)
    fx, fy = ux - fl_x, uy - fl_y
    i0, j0 = fl_x.astype(np.int64), fl_y.astype(np.int64)
    gx, gy = 1.0 - fx, 1.0 - fy
    w00, w10, w01, w11 = gx * gy, fx * gy, gx * fy, fx * fy
    m00, m10 = moments[probe, _texel(R, i0, j0)], moments[probe, _texel(R, i0 + 1, j0)]
    m01, m11 = moments[probe, _texel(R, i0, j0 + 1)], moments[probe, _texel(R, i0 + 1, j0 + 1)]
    with np.errstate(all="ignore"):
        val = ((w00[:, None] * m00 + w10[:, None] * m10) + w01[:, None] * m01) + w11[:, None] * m11
    return val[:, 0], val[:, 1]


def _texel_scalar(R, i, j):
    if i < 0 or i > R - 1:
        i = 0 if i < 0 else R - 1
        j = R - 1 - j
    if j < 0 or j > R - 1:
        j = 0 if j < 0 else R - 1
        i = R - 1 - i
    return i + R * j


def _mul(a, b):
    return float(np.float64(a) * np.float64(b))


def _add(a, b):
    return float(np.float64(a) + np.float64(b))


def _div(a, b):
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def lookup_scalar(probe_map, R, v):
    """probe_map [R*R, 2], v three floats (not zero) -> (mean, mean2)"""
    s = (abs(v[0]) + abs(v[1])) + abs(v[2])
    a, b = _div(v[0], s), _div(v[1], s)
    if v[2] < 0.0:
        a, b = (1.0 - abs(b)) * (1.0 if a >= 0.0 else -1.0), (1.0 - abs(a)) * (1.0 if b >= 0.0 else -1.0)
    idx, frac = [], []
    for c in (a, b):
        u = _mul(_add(_mul(c, 0.5), 0.5), float(R)) - 0.5
        u = u if u >= -0.5 else -0.5
        top = float(R) - 0.5
        u = u if u <= top else top
        fl = math.floor(u)
        idx.append(int(fl))
        frac.append(u - float(fl))
    (i0, j0), (fx, fy) = idx, frac
    gx, gy = 1.0 - fx, 1.0 - fy
    w = (gx * gy, fx * gy, gx * fy, fx * fy)
    t = (_texel_scalar(R, i0, j0), _texel_scalar(R, i0 + 1, j0), _texel_scalar(R, i0, j0 + 1), _texel_scalar(R, i0 + 1, j0 + 1))
    out = []
    for k in range(2):
        m = [float(probe_map[t[c]][k]) for c in range(4)]
        out.append(_add(_add(_add(_mul(w[0], m[0]), _mul(w[1], m[1])), _mul(w[2], m[2])), _mul(w[3], m[3])))
    return out[0], out[1]


# ---- the depth fold and the resolve -----------------------------------------------------------------------------------------------------
def fold(rays, status, t, samples, vis):
    """rays [N*S, 6], the query's status words [N*S] and t [N*S] -> (sums float64 [N, R*R, 3] of (W, M1, M2), probe status uint32 [N])"""
    rays = np.asarray(rays, dtype=np.float64).reshape(-1, samples, 6)
    status = np.asarray(status).reshape(-1, samples).astype(np.int64) & 0xFFFFFFFF
    t = np.asarray(t, dtype=np.float64).reshape(-1, samples)
    e = texel_dirs(vis.res)
    n = rays.shape[0]
    sums = np.zeros((n, vis.res * vis.res, 3))
    with np.errstate(all="ignore"):
        for s in range(samples):
            d = rays[:, s, 3:6]
            c = (d[:, None, 0] * e[None, :, 0] + d[:, None, 1] * e[None, :, 1]) + d[:, None, 2] * e[None, :, 2]
            w = np.where(c > 0.0, c, 0.0)
            for _ in range(vis.sharp):
                w = w * w
            dist = np.where(status[:, s] == 1, np.where(t[:, s] < vis.d_max, t[:, s], vis.d_max), vis.d_max)[:, None]
            sums[:, :, 0] = sums[:, :, 0] + w
            sums[:, :, 1] = sums[:, :, 1] + w * dist
            sums[:, :, 2] = sums[:, :, 2] + w * (dist * dist)
    bad = (status == 2).any(axis=1)
    sums[bad] = QNAN
    return sums, np.where(bad, 2, 1).astype(np.uint32)


def fold_scalar(rays, status, t, samples, vis, probe, tx, ty):
    """one (probe, texel) -> (W, M1, M2)"""
    e = texel_dir_scalar(vis.res, tx, ty)
    W = M1 = M2 = 0.0
    bad = False
    for k in range(probe * samples, (probe + 1) * samples):
        d = [float(x) for x in rays[k][3:6]]
        c = (d[0] * e[0] + d[1] * e[1]) + d[2] * e[2]
        w = c if c > 0.0 else 0.0
        for _ in range(vis.sharp):
            w = w * w
        st = int(status[k]) & 0xFFFFFFFF
        dist = (float(t[k]) if float(t[k]) < vis.d_max else vis.d_max) if st == 1 else vis.d_max
        W = W + w
        M1 = M1 + w * dist
        M2 = M2 + w * (dist * dist)
        bad |= st == 2
    return (float("nan"),) * 3 if bad else (W, M1, M2)


def resolve(sums, d_max):
    """-> moments float64 [N, R*R, 2]"""
    W, M1, M2 = sums[..., 0], sums[..., 1], sums[..., 2]
    with np.errstate(all="ignore"):
        mean = np.where(W > 0.0, M1 / W, d_max)
        mean2 = np.where(W > 0.0, M2 / W, d_max * d_max)
    nan = np.isnan(W)
    return np.stack([np.where(nan, W, mean), np.where(nan, W, mean2)], axis=-1)


def resolve_scalar(W, M1, M2, d_max):
    if W != W:
        return W, W
    return (_div(M1, W), _div(M2, W)) if W > 0.0 else (d_max, d_max * d_max)


# ---- the shade ------------------------------------------------------------------------------------------------------------------------------
def vis_weight(vis, r, q, mean, mean2):
    """step 3's extension for arrays: r = sqrt(q), the looked-up moments -> vis_w"""
    with np.errstate(all="ignore"):
        var = np.abs(mean * mean - mean2)
        d = r - mean
        ch = var / (var + d * d)
        ch = (ch * ch) * ch
        w = np.where(r > mean, np.where(ch > vis.floor, ch, vis.floor), 1.0)
        w = np.where(np.isnan(mean) | np.isnan(mean2), QNAN, w)
    return np.where(q > 0.0, w, 1.0)


def shade_vis(grid, vis, coeff, moments, points, normals, status=None, albedo=None, add=None, weights=False):
    """-> (irradiance float64 [m, 3], color float32 [m, 3]) by rt_hip_probe_shade's seven steps with step 3 extended; weights: also the
    vis_w of every (entry, corner) [m, 8], NaN where the corner was skipped"""
    coeff = np.asarray(coeff, dtype=np.float64).reshape(-1, 9, 3)
    moments = np.asarray(moments, dtype=np.float64).reshape(coeff.shape[0], vis.res * vis.res, 2)
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    n = np.asarray(normals, dtype=np.float64).reshape(-1, 3)
    m = len(p)
    miss = np.zeros(m, dtype=bool) if status is None else (np.asarray(status).reshape(-1).astype(np.int64) & 0xFFFFFFFF) != 1
    finite = np.isfinite(p).all(axis=1) & np.isfinite(n).all(axis=1)
    valid = ~miss & finite
    p = np.where(valid[:, None], p, 0.0)
    n = np.where(valid[:, None], n, 0.0)
    cells = _cells(grid, p)
    nx, ny, _ = grid.count
    B = np.zeros((m, 9, 3))
    W = np.zeros(m)
    seen = np.full((m, 8), np.nan)
    with np.errstate(all="ignore"):
        pb = p + n * vis.bias
        for c in range(8):
            b = (c & 1, (c >> 1) & 1, c >> 2)
            idx = [cells[a][b[a]] for a in range(3)]
            corner = [grid.origin[a] + idx[a].astype(np.float64) * grid.step[a] for a in range(3)]
            w = (cells[0][2 + b[0]] * cells[1][2 + b[1]]) * cells[2][2 + b[2]]
            if grid.flags & FACING:
                v = [corner[a] - p[:, a] for a in range(3)]
                q = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]
                cs = np.where(q > 0.0, ((v[0] * n[:, 0] + v[1] * n[:, 1]) + v[2] * n[:, 2]) * (1.0 / np.sqrt(q)), 1.0)
                s = (cs + 1.0) * 0.5
                w = w * (s * s + FACE_FLOOR)
            take = ~(w == 0.0)   # a NaN weight does not skip
            i = (idx[2] * ny + idx[1]) * nx + idx[0]
            v = np.stack([pb[:, a] - corner[a] for a in range(3)], axis=1)
            q = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
            mean, mean2 = lookup(moments, i, vis.res, v)
            vw = vis_weight(vis, np.sqrt(q), q, mean, mean2)
            seen[:, c] = np.where(take, vw, np.nan)
            w = w * vw
            B = np.where(take[:, None, None], B + (w[:, None, None] * coeff[i]), B)
            W = np.where(take, W + w, W)
        basis = sh_bases(n)
        E = np.zeros((m, 3))
        for j in range(9):
            E = E + (A[j] * B[:, j, :]) * basis[:, j, None]
        E = E / W[:, None]
        E = np.where(E < 0.0, 0.0, E)
        alb = np.ones((m, 3), dtype=np.float32) if albedo is None else np.asarray(albedo, dtype=np.float32).reshape(-1, 3)
        ad = np.zeros((m, 3), dtype=np.float32) if add is None else np.asarray(add, dtype=np.float32).reshape(-1, 3)
        color = (((alb.astype(np.float64) * E) * INV_PI) + ad.astype(np.float64)).astype(np.float32)
        miss_color = (np.array(grid.miss_color, dtype=np.float64)[None, :] + ad.astype(np.float64)).astype(np.float32)
    E[miss] = 0.0
    color[miss] = miss_color[miss]
    bad = ~miss & ~finite
    E[bad] = QNAN
    color[bad] = np.float32("nan")
    return (E, color, seen) if weights else (E, color)


def shade_vis_scalar(grid, vis, coeff, moments, p, n, status=None, albedo=None, add=None):
    """one entry -> (E three floats, color three numpy float32), one double at a time"""
    ad = [0.0, 0.0, 0.0] if add is None else [float(np.float32(x)) for x in add]
    if status is not None and int(status) & 0xFFFFFFFF != 1:
        return [0.0] * 3, [np.float32(grid.miss_color[ch] + ad[ch]) for ch in range(3)]
    p, n = [float(x) for x in p], [float(x) for x in n]
    if not all(math.isfinite(x) for x in p + n):
        return [float("nan")] * 3, [np.float32("nan")] * 3
    idx, wts = [], []
    for a in range(3):
        N = grid.count[a]
        g = _div(p[a] - grid.origin[a], grid.step[a])
        g = g if g > 0.0 else 0.0
        top = float(N - 1)
        g = g if g < top else top
        i0 = int(g)
        if N >= 2 and i0 > N - 2:
            i0 = N - 2
        f = g - float(i0)
        idx.append((i0, i0 + 1 if N >= 2 else 0))
        wts.append((1.0 - f, f))
    nx, ny, _ = grid.count
    R = vis.res
    B = [[0.0] * 3 for _ in range(9)]
    W = 0.0
    pb = [_add(p[a], _mul(n[a], vis.bias)) for a in range(3)]
    with np.errstate(all="ignore"):
        for c in range(8):
            b = (c & 1, (c >> 1) & 1, c >> 2)
            i = [idx[a][b[a]] for a in range(3)]
            corner = [_add(grid.origin[a], _mul(float(i[a]), grid.step[a])) for a in range(3)]
            w = (wts[0][b[0]] * wts[1][b[1]]) * wts[2][b[2]]
            if grid.flags & FACING:
                v = [np.float64(corner[a]) - p[a] for a in range(3)]
                q = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]
                cs = ((v[0] * n[0] + v[1] * n[1]) + v[2] * n[2]) * (1.0 / np.sqrt(q)) if q > 0.0 else 1.0
                s = (cs + 1.0) * 0.5
                w = float(w * (s * s + FACE_FLOOR))
            if w == 0.0:
                continue
            probe = (i[2] * ny + i[1]) * nx + i[0]
            v = [float(np.float64(pb[a]) - np.float64(corner[a])) for a in range(3)]
            q = float((np.float64(v[0]) * v[0] + np.float64(v[1]) * v[1]) + np.float64(v[2]) * v[2])
            vis_w = 1.0
            if q > 0.0:
                r = float(np.sqrt(np.float64(q)))
                mean, mean2 = lookup_scalar(moments[probe], R, v)
                if r > mean:
                    var = abs(_add(_mul(mean, mean), -mean2))
                    d = r - mean
                    ch = _div(var, _add(var, _mul(d, d)))
                    ch = _mul(_mul(ch, ch), ch)
                    vis_w = ch if ch > vis.floor else vis.floor
                if mean != mean or mean2 != mean2:
                    vis_w = float("nan")
            w = _mul(w, vis_w)
            pc = coeff[probe]
            for j in range(9):
                for ch in range(3):
                    B[j][ch] = float(np.float64(B[j][ch]) + (np.float64(w) * np.float64(pc[j][ch])))
            W = _add(W, w)
        E, color = [], []
        for ch in range(3):
            s = np.float64(0.0)
            for j in range(9):
                s = s + (np.float64(A[j]) * np.float64(B[j][ch])) * np.float64(sh_basis_scalar(j, *n))
            s = s / np.float64(W)
            s = np.float64(0.0) if s < 0.0 else s
            E.append(float(s))
            alb = 1.0 if albedo is None else float(np.float32(albedo[ch]))
            color.append(np.float32(((np.float64(alb) * s) * INV_PI) + np.float64(ad[ch])))
    return E, color


# ---- what the CPU and the GPU tests share -------------------------------------------------------------------------------------------------
def random_moments(grid, vis, seed=9):
    """random moments [n, R*R, 2] about the grid's scale: means from well below the distances of a cell to well above them, so that
    both sides of r > mean occur, mean2 = mean^2 plus a variance of either size; a few texels with mean2 < mean^2 (var is an absolute
    value) and a few with zero variance"""
    rng = np.random.default_rng(seed)
    scale = math.sqrt(sum(s * s for s in grid.step))
    mean = scale * (0.05 + 1.5 * rng.random((grid.n, vis.res * vis.res)))
    var = (scale * scale) * rng.random(mean.shape) ** 3
    var[rng.random(mean.shape) < 0.05] *= -0.5
    var[rng.random(mean.shape) < 0.05] = 0.0
    return np.stack([mean, mean * mean + var], axis=-1)

"""The light probes of include/rt_hip.h ("light probes") restated on the CPU, twice: one numpy form, vectorised over rays, and one
plain scalar Python form of the same text, one double at a time.  rt_rng.h's generator is tests/lens_expected.py's.  Python floats and
numpy float64 are IEEE doubles, + - * / and sqrt correctly rounded and never fused: what the contract asks of the device.  The ray of
index k, the bases, the fold, the resolve, the irradiance from SH9, and the cases the tests share.
"""
import math

import numpy as np

from lens_expected import M64, Stream, draw_v, mix64, rng_seed_v

PROBE_KEY = 0x70726F62
ROUNDS = 32
Q_MIN = 2.0 ** -20
SPHERE, HEMISPHERE = 0, 1
BASES = {SPHERE: 9, HEMISPHERE: 1}
Y0, Y1, Y2A, Y2B, Y2C = 0.28209479177387814, 0.4886025119029199, 1.0925484305920792, 0.31539156525252005, 0.5462742152960396
K = {SPHERE: 12.566370614359172, HEMISPHERE: 6.283185307179586}
A = (3.141592653589793,) + (2.0943951023931953,) * 3 + (0.7853981633974483,) * 5
QNAN = np.uint64(0x7FF8000000000000).view(np.float64)


# ---- the ray, scalar --------------------------------------------------------------------------------------------------------------------
def probe_ray_scalar(positions, normals, samples, seed, k, bias=0.0, draw=None):
    """the ray of index k -> (six floats, rounds that did not accept).  normals None: a sphere probe.  draw: a function that gives
    the stream's next double in the stream's place (for the all-reject path)"""
    i = k // samples
    if draw is None:
        draw = Stream(mix64((seed ^ PROBE_KEY) & M64), k, 0).draw
    d, rejected = (0.0, 0.0, 1.0), ROUNDS
    for rnd in range(ROUNDS):
        r1, r2, r3 = draw(), draw(), draw()
        x, y, z = r1 * 2.0 + -1.0, r2 * 2.0 + -1.0, r3 * 2.0 + -1.0
        q = (x * x + y * y) + z * z
        if q <= 1.0 and q >= Q_MIN:
            inv = 1.0 / math.sqrt(q)
            d, rejected = (x * inv, y * inv, z * inv), rnd
            break
    o = tuple(float(c) for c in positions[i])
    if normals is not None:
        n = tuple(float(c) for c in normals[i])
        with np.errstate(all="ignore"):
            c = float((np.float64(d[0]) * n[0] + np.float64(d[1]) * n[1]) + np.float64(d[2]) * n[2])
            if c < 0:
                d = (d[0] * -1.0, d[1] * -1.0, d[2] * -1.0)
            o = tuple(float(np.float64(o[a]) + np.float64(n[a]) * bias) for a in range(3))
    return o + d, rejected


# ---- the ray, numpy ---------------------------------------------------------------------------------------------------------------------
def probe_rays(positions, normals, samples, seed, k_first=0, n=None, bias=0.0, info=False):
    """the rays of indices [k_first, k_first + n) -> float64 [n, 6] (and, with info, the rounds that did not accept, int64 [n])"""
    positions = np.asarray(positions, dtype=np.float64).reshape(-1, 3)
    total = positions.shape[0] * samples
    n = total - k_first if n is None else n
    k = k_first + np.arange(n, dtype=np.int64)
    i = k // samples
    state = rng_seed_v(mix64((seed ^ PROBE_KEY) & M64), k, 0)
    d = np.tile(np.array([0.0, 0.0, 1.0]), (n, 1))
    rejected = np.full(n, ROUNDS, dtype=np.int64)
    waiting = np.ones(n, dtype=bool)
    for rnd in range(ROUNDS):
        if not waiting.any():
            break
        state, r1 = draw_v(state)
        state, r2 = draw_v(state)
        state, r3 = draw_v(state)
        x, y, z = r1 * 2.0 + -1.0, r2 * 2.0 + -1.0, r3 * 2.0 + -1.0
        q = (x * x + y * y) + z * z
        take = waiting & (q <= 1.0) & (q >= Q_MIN)
        with np.errstate(all="ignore"):
            inv = 1.0 / np.sqrt(q)
        for a, v in enumerate((x, y, z)):
            d[take, a] = (v * inv)[take]
        rejected[take] = rnd
        waiting &= ~take
    o = positions[i] if n else np.zeros((0, 3))
    if normals is not None and n:
        nn = np.asarray(normals, dtype=np.float64).reshape(-1, 3)[i]
        with np.errstate(all="ignore"):
            c = (d[:, 0] * nn[:, 0] + d[:, 1] * nn[:, 1]) + d[:, 2] * nn[:, 2]
            d = np.where((c < 0)[:, None], d * -1.0, d)
            o = o + nn * bias
    rays = np.concatenate([o, d], axis=1)
    return (rays, rejected) if info else rays


# ---- the bases ------------------------------------------------------------------------------------------------------------------------
def sh_basis_scalar(j, x, y, z):
    return (Y0, Y1 * y, Y1 * z, Y1 * x, Y2A * (x * y), Y2A * (y * z), Y2B * (3.0 * (z * z) - 1.0), Y2A * (x * z), Y2C * (x * x - y * y))[j]


def sh_bases(d):
    """directions [n, 3] -> w [n, 9]"""
    d = np.asarray(d, dtype=np.float64).reshape(-1, 3)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    with np.errstate(all="ignore"):
        return np.stack([np.full(len(d), Y0), Y1 * y, Y1 * z, Y1 * x, Y2A * (x * y), Y2A * (y * z), Y2B * (3.0 * (z * z) - 1.0),
                         Y2A * (x * z), Y2C * (x * x - y * y)], axis=1)


def cos_basis(d, n):
    """directions [m, 3], normals [m, 3] -> w [m, 1]: the clamped cosine (a NaN reads 0)"""
    d, n = np.asarray(d, dtype=np.float64).reshape(-1, 3), np.asarray(n, dtype=np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        c = (d[:, 0] * n[:, 0] + d[:, 1] * n[:, 1]) + d[:, 2] * n[:, 2]
        return np.where(c > 0, c, 0.0)[:, None]


def weights(rays, samples, normals=None):
    """the rays of whole probes [N * S, 6] -> w [N * S, bases]"""
    if normals is None:
        return sh_bases(rays[:, 3:])
    return cos_basis(rays[:, 3:], np.repeat(np.asarray(normals, dtype=np.float64).reshape(-1, 3), samples, axis=0))


# ---- the fold, the resolve ------------------------------------------------------------------------------------------------------------------
def fold(rays, radiance, samples, normals=None, statuses=None):
    """whole probes: rays [N * S, 6], radiance [N * S, 3] -> sums [N, bases, 3]: per (probe, basis, channel) in ascending k from +0.0,
    sum = sum + (radiance * w); a status-2 ray makes its probe's sums NaN"""
    w = weights(rays, samples, normals)
    n = len(rays) // samples
    w = w.reshape(n, samples, -1)
    rad = np.asarray(radiance, dtype=np.float64).reshape(n, samples, 3)
    total = np.zeros((n, w.shape[2], 3))
    with np.errstate(all="ignore"):
        for s in range(samples):
            total = total + rad[:, s, None, :] * w[:, s, :, None]
    if statuses is not None:
        total[(np.asarray(statuses).reshape(n, samples) == 2).any(axis=1)] = QNAN
    return total


def fold_scalar(rays, radiance, samples, probe, j, c, normals=None):
    """one sum of fold(), one double at a time (valid rays)"""
    total = 0.0
    for k in range(probe * samples, (probe + 1) * samples):
        x, y, z = (float(v) for v in rays[k][3:])
        if normals is None:
            w = sh_basis_scalar(j, x, y, z)
        else:
            n = [float(v) for v in normals[probe]]
            cs = (x * n[0] + y * n[1]) + z * n[2]
            w = cs if cs > 0 else 0.0
        total = total + float(radiance[k][c]) * w
    return total


def resolve(total, samples, mode):
    """-> (coeff float64, coeff_f float32)"""
    with np.errstate(all="ignore"):
        coeff = (np.asarray(total, dtype=np.float64) * (1.0 / float(samples))) * K[mode]
        return coeff, coeff.astype(np.float32)


# ---- irradiance from SH9 ------------------------------------------------------------------------------------------------------------------
def irradiance(coeff, index, normals):
    """coeff [N, 9, 3], index [m], normals [m, 3] -> E [m, 3]: ascending over j from +0.0 of (A_j * coeff) * w_j(n); NaN for index >= N"""
    coeff = np.asarray(coeff, dtype=np.float64).reshape(-1, 9, 3)
    index = np.asarray(index, dtype=np.int64)
    ok = index < len(coeff)
    w = sh_bases(normals)
    E = np.zeros((len(index), 3))
    picked = coeff[np.where(ok, index, 0)] if len(coeff) else np.zeros((len(index), 9, 3))
    with np.errstate(all="ignore"):
        for j in range(9):
            E = E + (A[j] * picked[:, j, :]) * w[:, j, None]
    E[~ok] = QNAN
    return E


def irradiance_scalar(coeff, i, n, c):
    if i >= len(coeff):
        return float("nan")
    E = 0.0
    with np.errstate(all="ignore"):
        for j in range(9):
            E = E + float(np.float64(A[j]) * np.float64(coeff[i][j][c])) * sh_basis_scalar(j, *n)
    return E


# ---- the cases the CPU and the GPU tests share -------------------------------------------------------------------------------------------
SEED = 20261020
SETS = ((1, 1), (1, 63), (1, 64), (1, 65), (5, 13), (200, 3))   # (N, S)
BIASES = (0.0, 2.0 ** -10)
DISTANCES = (1e-3, 1.0, 1e6)


def positions(n, distance):
    """n points at `distance` from the origin, no two alike"""
    t = np.arange(n, dtype=np.float64)
    v = np.stack([np.cos(0.7 * t + 0.3), np.sin(1.3 * t + 0.1), np.cos(2.1 * t) * 0.5 + 0.25], axis=1)
    return v / np.linalg.norm(v, axis=1)[:, None] * distance


def normals(n):
    """n normals, used as given: unit to rounding but for every fourth, which is twice as long"""
    t = np.arange(n, dtype=np.float64)
    v = np.stack([np.sin(0.9 * t + 1.0), np.cos(0.4 * t), np.sin(1.7 * t + 2.0)], axis=1)
    v = v / np.linalg.norm(v, axis=1)[:, None]
    v[3::4] *= 2.0
    return v


def sub_ranges(n_probes, samples):
    """(k_first, n): the whole set, empty ranges, ranges that start and end inside a wave, ranges that span probe boundaries"""
    total = n_probes * samples
    out = [(0, total), (0, 0), (total, 0)]
    if total > 8:
        out += [(3, total - 5), (1, 1)]
    if total > 80:
        out += [(7, 64), (70, total - 75)]
    if n_probes > 1:
        out += [(samples - 1, 2), (samples - 1, samples + 2)]
    return out


# ---- the furnace (tests/test_gpu_probe.py bakes it; the CPU derives what it must give) --------------------------------------------------------
# One sphere of radius 1000 and colour 0 that emits: the roulette ends every path at its first hit, so a sample that hits IS the
# emission.  The reference's sphere test (raytracer.c:82-85) misses when tca = (centre - origin) . d < 0, also from inside the sphere:
# a probe AT the centre (tca = +-0) hits with every ray, one off the centre sees the background (10 / 255) in the directions that
# point away from it.  Either way the CPU knows every sample.  Three probes at the centre, three within 10 of it.
FURNACE = dict(emission=(1.0, 0.5, 0.25), samples=64, depth=4, n=6, central=3)
BACKGROUND = 10 / 255.0


def furnace_scene():
    from rt_amd import abi, scene as S
    objs = [dict(flags=abi.M_DEFAULT, radius=1000.0, center=(0.0, 0.0, 0.0), color=(0.0, 0.0, 0.0), emission=FURNACE["emission"])]
    return S.custom_scene(objs, 16, 16, 1, FURNACE["depth"], (0.0, 0.0, 10.0), (0.0, 0.0, 0.0))


def furnace_positions():
    return positions(FURNACE["n"], 1.0) * np.array([0.0, 0.0, 0.0, 1e-3, 3.0, 10.0])[:, None]


def furnace_radiance(rays):
    """the sample of each ray: the emission where intersect_sphere's tca = vec3_dot(centre - origin, d) is not negative"""
    L = 0.0 - rays[:, :3]
    d = rays[:, 3:]
    tca = (L[:, 0] * d[:, 0] + L[:, 1] * d[:, 1]) + L[:, 2] * d[:, 2]
    return np.where((tca < 0)[:, None], BACKGROUND, np.array(FURNACE["emission"])[None, :])

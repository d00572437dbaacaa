"""The probe updates of include/rt_hip.h ("probe updates") restated on the CPU, twice: one numpy form, vectorised, and one plain scalar
Python form of the same text, one double at a time.  Python floats and numpy float64 are IEEE doubles, + - * / correctly rounded and
never fused: what the contract asks of the device.  The round's probes and seed, alpha, the two blends and the age step; the rays,
the folds and the resolves are tests/probe_expected.py's and tests/probe_vis_expected.py's.
"""
import numpy as np

from lens_expected import M64, mix64
from probe_expected import K, SPHERE

AGE_MAX = 0xFFFFFFFF


class Update:
    """an RtHipProbeUpdate's fields; the defaults are rt_hip_probe_update_defaults'"""

    def __init__(self, stride=1, phase=0, round=0, hysteresis=0.9, change=0.0, fast=0.0):
        self.stride, self.phase, self.round = int(stride), int(phase), int(round)
        self.hysteresis, self.change, self.fast = float(hysteresis), float(change), float(fast)

    def abi(self):
        from rt_amd import abi
        return abi.probe_update(self.stride, self.phase, self.round, self.hysteresis, self.change, self.fast)


# ---- the round ---------------------------------------------------------------------------------------------------------------------------
def count(n, stride, phase):
    """M: how many probes of n the round updates"""
    return (n - 1 - phase) // stride + 1 if phase < n else 0


def probes(n, stride, phase):
    """i_0 .. i_{M-1} as an int64 array"""
    return phase + stride * np.arange(count(n, stride, phase), dtype=np.int64)


def probes_scalar(n, stride, phase):
    """... one at a time, from the definition: the i below n with i % stride == phase, ascending"""
    return [i for i in range(n) if i % stride == phase]


def round_seed(seed, round):
    """seed_u = rt_mix64(seed + round), the add wrapping"""
    return mix64((seed + round) & M64)


# ---- alpha -------------------------------------------------------------------------------------------------------------------------------
def alpha(age, h):
    age = np.asarray(age).astype(np.int64) & AGE_MAX
    warm = 1.0 / (age.astype(np.float64) + 1.0)
    base = 1.0 - h
    return np.where(warm > base, warm, base)


def alpha_scalar(age, h):
    warm = 1.0 / (float(int(age) & AGE_MAX) + 1.0)
    base = 1.0 - h
    return warm if warm > base else base


# ---- the coefficient blend -----------------------------------------------------------------------------------------------------------------
def blend_coeff(total, samples, upd, age, coeff, change=None):
    """total [M, 9, 3] the round's fresh sums, age [N], coeff [N, 9, 3] the old state, change [N] or None ->
    (coeff, coeff_f float32, change) after the round; the inputs are left as they are"""
    coeff = np.array(coeff, dtype=np.float64)
    n = coeff.shape[0]
    change = np.zeros(n) if change is None else np.array(change, dtype=np.float64)
    idx = probes(n, upd.stride, upd.phase)
    if len(idx) == 0:
        return coeff, coeff.astype(np.float32), change
    with np.errstate(all="ignore"):
        fresh = (np.asarray(total, dtype=np.float64).reshape(len(idx), 9, 3) * (1.0 / float(samples))) * K[SPHERE]
        old = coeff[idx]
        a = alpha(np.asarray(age)[idx], upd.hysteresis)
        over = (np.asarray(age)[idx].astype(np.int64) & AGE_MAX) == 0   # the probe starts over
        c, m = np.zeros(len(idx)), np.zeros(len(idx))
        for ch in range(3):
            f, o = fresh[:, 0, ch], old[:, 0, ch]
            d = np.abs(f - o)
            c = np.where(d > c, d, c)
            af, ao = np.abs(f), np.abs(o)
            g = np.where(af > ao, af, ao)
            m = np.where(g > m, g, m)
        rel = np.where(m > 0.0, c / np.where(m > 0.0, m, 1.0), 0.0)
        quick = 1.0 - upd.fast
        lifted = np.where(a > quick, a, quick)
        a2 = np.where((upd.change > 0.0) & (c > upd.change * m), lifted, a)
        keep = 1.0 - a2
        blended = (old * keep[:, None, None]) + (fresh * a2[:, None, None])
    out = np.where(over[:, None, None], fresh, blended)
    coeff[idx] = out
    change[idx] = np.where(over, 1.0, rel)
    with np.errstate(all="ignore"):
        return coeff, coeff.astype(np.float32), change


def blend_coeff_scalar(total_j, samples, upd, age_i, old_i):
    """one probe: total_j [9][3], its age, old_i [9][3] -> (out [9][3], change_out)"""
    inv = 1.0 / float(samples)
    fresh = [[_mul(_mul(float(total_j[b][ch]), inv), K[SPHERE]) for ch in range(3)] for b in range(9)]
    a = alpha_scalar(age_i, upd.hysteresis)
    if int(age_i) & AGE_MAX == 0:
        return fresh, 1.0
    c = m = 0.0
    for ch in range(3):
        f, o = fresh[0][ch], float(old_i[0][ch])
        d = abs(_sub(f, o))
        c = d if d > c else c
        g = abs(f) if abs(f) > abs(o) else abs(o)
        m = g if g > m else m
    change_out = _div(c, m) if m > 0.0 else 0.0
    if upd.change > 0.0 and c > _mul(upd.change, m):
        quick = 1.0 - upd.fast
        a = a if a > quick else quick
    keep = 1.0 - a
    return [[_add(_mul(float(old_i[b][ch]), keep), _mul(fresh[b][ch], a)) for ch in range(3)] for b in range(9)], change_out


# ---- the moment blend ----------------------------------------------------------------------------------------------------------------------
def blend_moments(sums, d_max, upd, age, moments):
    """sums [M, T, 3] the round's fresh (W, M1, M2), age [N], moments [N, T, 2] the old state -> moments after the round"""
    moments = np.array(moments, dtype=np.float64)
    idx = probes(moments.shape[0], upd.stride, upd.phase)
    if len(idx) == 0:
        return moments
    sums = np.asarray(sums, dtype=np.float64).reshape(len(idx), moments.shape[1], 3)
    W, M1, M2 = sums[..., 0], sums[..., 1], sums[..., 2]
    a = alpha(np.asarray(age)[idx], upd.hysteresis)[:, None]
    keep = 1.0 - a
    old = moments[idx]
    over = ((np.asarray(age)[idx].astype(np.int64) & AGE_MAX) == 0)[:, None]
    out = np.empty_like(old)
    with np.errstate(all="ignore"):
        safe = np.where(W > 0.0, W, 1.0)
        for k, (num, empty) in enumerate(((M1, d_max), (M2, d_max * d_max))):
            f = num / safe
            hit = np.where(over, f, (old[..., k] * keep) + (f * a))
            silent = np.where(over, empty, old[..., k])
            out[..., k] = np.where(np.isnan(W), W, np.where(W > 0.0, hit, silent))
    moments[idx] = out
    return moments


def blend_moments_scalar(W, M1, M2, d_max, upd, age_i, old):
    """one texel: its fresh sums, the probe's age, old (mean, mean2) -> (mean, mean2)"""
    a = alpha_scalar(age_i, upd.hysteresis)
    if W != W:
        return W, W
    if W > 0.0:
        f = (_div(M1, W), _div(M2, W))
        if int(age_i) & AGE_MAX == 0:
            return f
        keep = 1.0 - a
        return tuple(_add(_mul(float(old[k]), keep), _mul(f[k], a)) for k in range(2))
    return (d_max, d_max * d_max) if int(age_i) & AGE_MAX == 0 else (float(old[0]), float(old[1]))


# ---- the age step --------------------------------------------------------------------------------------------------------------------------
def age_step(age, upd):
    age = np.array(age).astype(np.int64) & AGE_MAX
    idx = probes(len(age), upd.stride, upd.phase)
    age[idx] = np.where(age[idx] == AGE_MAX, age[idx], age[idx] + 1)
    return age.astype(np.uint32)


def age_step_scalar(a):
    a = int(a) & AGE_MAX
    return a if a == AGE_MAX else a + 1


def _mul(a, b):
    with np.errstate(all="ignore"):
        return float(np.float64(a) * np.float64(b))


def _add(a, b):
    with np.errstate(all="ignore"):
        return float(np.float64(a) + np.float64(b))


def _sub(a, b):
    with np.errstate(all="ignore"):
        return float(np.float64(a) - np.float64(b))


def _div(a, b):
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


# ---- crafted inputs, shared by the CPU and the GPU tests ------------------------------------------------------------------------------------
AGES = (0, 1, 9, 10, AGE_MAX - 1, AGE_MAX)


def crafted_state(n, texels, seed=3):
    """A state of n probes whose ages walk AGES and whose old values are NaN exactly where the age is 0 ->
    (age uint32 [n], coeff [n, 9, 3], moments [n, texels, 2], change [n])"""
    rng = np.random.default_rng(seed)
    age = np.array([AGES[i % len(AGES)] for i in range(n)], dtype=np.uint32)
    coeff = rng.uniform(-1.0, 2.0, (n, 9, 3))
    mean = rng.uniform(0.1, 3.0, (n, texels))
    moments = np.stack([mean, mean * mean + rng.uniform(0.0, 0.5, (n, texels))], axis=-1)
    coeff[age == 0] = np.nan
    moments[age == 0] = np.nan
    return age, coeff, moments, rng.uniform(0.0, 1.0, n)


def crafted_sums(m, samples, seed=4):
    """fresh sums [m, 9, 3] with a NaN, both zeros and 1e300 among random values"""
    rng = np.random.default_rng(seed)
    total = rng.uniform(-1.0, 2.0, (m, 9, 3)) * samples / K[SPHERE]
    flat = total.reshape(-1)
    if m == 0:
        return total
    for k, v in enumerate((np.nan, 0.0, -0.0, 1e300, -1e300)):
        flat[(7 * k + 5) % flat.size::max(flat.size // 3, 1)] = v
    if m > 2:
        total[2, 0, :] = (0.0, -0.0, 0.0)   # an L0 band of zeros: m may be 0
    return total


def crafted_depth_sums(m, texels, seed=6):
    """fresh (W, M1, M2) [m, texels, 3] with W of 0, NaN and a denormal among random values"""
    rng = np.random.default_rng(seed)
    W = rng.uniform(0.01, 4.0, (m, texels))
    dist = rng.uniform(0.1, 3.0, (m, texels))
    sums = np.stack([W, W * dist, W * dist * dist], axis=-1)
    flat = sums.reshape(-1, 3)
    flat[1::5] = (0.0, 0.0, 0.0)
    flat[3::11] = (5e-324, 1e-323, 2e-323)
    flat[2::13] = (np.nan, np.nan, np.nan)
    flat[4::17, 0] = -0.0
    return sums


def threshold_case(change, samples):
    """Old values and fresh sums whose c sits on the fast rule's threshold c == change * m, and one ulp either side of it -> list of
    (old [9, 3], total [9, 3], side -1 | 0 | +1).  Channel 1 of band 0 does not move and sets m = |fresh|; channel 0's fresh value
    is 0.0 and its old value c itself, so that c = |0.0 - old| is exact."""
    out = []
    total = np.full((9, 3), 0.375 * samples)
    total[0] = (0.0, 1.75 * samples, 0.0)
    f1 = _mul(_mul(total[0][1], 1.0 / float(samples)), K[SPHERE])
    c0 = _mul(change, f1)
    for side, c in ((-1, float(np.nextafter(c0, 0.0))), (0, c0), (1, float(np.nextafter(c0, np.inf)))):
        old = np.full((9, 3), 0.5)
        old[0] = (c, f1, 0.0)
        out.append((old, total.copy(), side))
    return out

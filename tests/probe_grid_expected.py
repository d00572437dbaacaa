"""The probe grids of include/rt_hip.h ("probe grids") restated on the CPU, twice: one numpy form, vectorised over entries, and one
plain scalar Python form of the same text, one double at a time.  Python floats and numpy float64 are IEEE doubles, + - * / and sqrt
correctly rounded and never fused: what the contract asks of the device.  The constants and the basis are tests/probe_expected.py's.
The grid's positions, the shade, and the entries the CPU and the GPU tests share.
"""
import math

import numpy as np

from probe_expected import A, QNAN, sh_bases, sh_basis_scalar

FACING = 1
INV_PI = 0.3183098861837907
FACE_FLOOR = 0.2
MISS_COLOR = float(np.float32(10.0 / 255.0))
COUNTS = ((1, 1, 1), (2, 3, 4), (5, 1, 2))
ORIGIN = (-0.35, 1e-3, 2.0)
STEP = (0.1, 0.3, 0.7)


class Grid:
    """an RtHipProbeGrid's fields"""

    def __init__(self, origin=ORIGIN, step=STEP, count=(2, 3, 4), flags=0, miss_color=(MISS_COLOR,) * 3):
        self.origin, self.step, self.count, self.flags = tuple(map(float, origin)), tuple(map(float, step)), tuple(map(int, count)), flags
        self.miss_color = tuple(float(np.float32(c)) for c in miss_color)

    @property
    def n(self):
        return self.count[0] * self.count[1] * self.count[2]

    def abi(self):
        from rt_amd import abi
        return abi.probe_grid(self.origin, self.step, self.count, facing=bool(self.flags & FACING), miss_color=self.miss_color)


def positions(grid):
    """-> float64 [n, 3]: origin + (double)i * step per axis, probe (ix, iy, iz) at index (iz * ny + iy) * nx + ix"""
    nx, ny, nz = grid.count
    i = np.arange(grid.n)
    idx = (i % nx, (i // nx) % ny, i // (nx * ny))
    return np.stack([grid.origin[a] + idx[a].astype(np.float64) * grid.step[a] for a in range(3)], axis=1)


# ---- the shade, numpy -------------------------------------------------------------------------------------------------------------------
def _cells(grid, p):
    """step 2 -> per axis (i0, i1, w0, w1)"""
    out = []
    for a in range(3):
        N = grid.count[a]
        with np.errstate(all="ignore"):
            g = (p[:, a] - grid.origin[a]) / grid.step[a]
            g = np.where(g > 0.0, g, 0.0)
            top = float(N - 1)
            g = np.where(g < top, g, top)
            i0 = g.astype(np.int64)
            if N >= 2:
                i0 = np.where(i0 > N - 2, N - 2, i0)
            f = g - i0.astype(np.float64)
        i1 = i0 + 1 if N >= 2 else np.zeros_like(i0)
        out.append((i0, i1, 1.0 - f, f))
    return out


def shade(grid, coeff, points, normals, status=None, albedo=None, add=None):
    """-> (irradiance float64 [m, 3], color float32 [m, 3]) by the contract's seven steps"""
    coeff = np.asarray(coeff, dtype=np.float64).reshape(-1, 9, 3)
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    n = np.asarray(normals, dtype=np.float64).reshape(-1, 3)
    m = len(p)
    miss = np.zeros(m, dtype=bool) if status is None else (np.asarray(status).reshape(-1).astype(np.int64) & 0xFFFFFFFF) != 1
    finite = np.isfinite(p).all(axis=1) & np.isfinite(n).all(axis=1)
    valid = ~miss & finite
    # INVALID and MISS entries are computed with a stand-in and overwritten below
    p = np.where(valid[:, None], p, 0.0)
    n = np.where(valid[:, None], n, 0.0)
    cells = _cells(grid, p)
    nx, ny, _ = grid.count
    B = np.zeros((m, 9, 3))
    W = np.zeros(m)
    with np.errstate(all="ignore"):
        for c in range(8):
            b = (c & 1, (c >> 1) & 1, c >> 2)
            idx = [cells[a][b[a]] for a in range(3)]
            w = (cells[0][2 + b[0]] * cells[1][2 + b[1]]) * cells[2][2 + b[2]]
            if grid.flags & FACING:
                v = [(grid.origin[a] + idx[a].astype(np.float64) * grid.step[a]) - p[:, a] for a in range(3)]
                q = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]
                cs = np.where(q > 0.0, ((v[0] * n[:, 0] + v[1] * n[:, 1]) + v[2] * n[:, 2]) * (1.0 / np.sqrt(q)), 1.0)
                s = (cs + 1.0) * 0.5
                w = w * (s * s + FACE_FLOOR)
            take = ~(w == 0.0)   # a NaN weight does not skip
            i = (idx[2] * ny + idx[1]) * nx + idx[0]
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
    return E, color


# ---- the shade, scalar ------------------------------------------------------------------------------------------------------------------
def _div(a, b):
    return float(np.float64(a) / np.float64(b))


def shade_scalar(grid, coeff, p, n, status=None, albedo=None, add=None):
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
    B = [[0.0] * 3 for _ in range(9)]
    W = 0.0
    with np.errstate(all="ignore"):
        for c in range(8):
            b = (c & 1, (c >> 1) & 1, c >> 2)
            i = [idx[a][b[a]] for a in range(3)]
            w = (wts[0][b[0]] * wts[1][b[1]]) * wts[2][b[2]]
            if grid.flags & FACING:
                v = [np.float64(grid.origin[a] + float(i[a]) * grid.step[a]) - p[a] for a in range(3)]
                q = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]
                cs = ((v[0] * n[0] + v[1] * n[1]) + v[2] * n[2]) * (1.0 / np.sqrt(q)) if q > 0.0 else 1.0
                s = (cs + 1.0) * 0.5
                w = float(w * (s * s + FACE_FLOOR))
            if w == 0.0:
                continue
            probe = coeff[(i[2] * ny + i[1]) * nx + i[0]]
            for j in range(9):
                for ch in range(3):
                    B[j][ch] = float(np.float64(B[j][ch]) + (np.float64(w) * np.float64(probe[j][ch])))
            W = W + w
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


# ---- the entries the CPU and the GPU tests share ------------------------------------------------------------------------------------------
def coefficients(grid, seed=5):
    """random fp64 coefficients of both signs, [n, 9, 3]"""
    return np.random.default_rng(seed).normal(0.0, 1.0, (grid.n, 9, 3))


def random_entries(grid, m, seed=7):
    """m points uniform in a box 1.5 x the grid about its centre, normals unit, zero (every 7th) and of length 1e3 (every 5th)"""
    rng = np.random.default_rng(seed)
    lo = np.array(grid.origin)
    span = np.array([(grid.count[a] - 1) * grid.step[a] for a in range(3)])
    span_or_step = np.where(span > 0, span, np.array(grid.step))
    centre = lo + 0.5 * span
    p = centre + (rng.random((m, 3)) - 0.5) * 1.5 * span_or_step
    n = rng.normal(size=(m, 3))
    n /= np.linalg.norm(n, axis=1)[:, None]
    n[::7] = 0.0
    n[3::5] *= 1e3
    return p, n


def edge_points(grid):
    """every clamp on every side, every probe position (recomputed by the formula: q == 0 there), cell faces and edges, 2^-40 to
    either side of a face, a run of 64 entries inside one cell and a run that alternates between two cells -> float64 [k, 3]"""
    pos = positions(grid)
    lo = np.array(grid.origin)
    hi = pos[-1]
    step = np.array(grid.step)
    mid = lo + 0.5 * (hi - lo)
    pts = [pos]
    for a in range(3):
        for far in (-3.0, -1e-9, 1e-9, 3.0):
            for base in (lo, hi):
                q = mid.copy()
                q[a] = base[a] + far * step[a]
                pts.append(q[None, :])
        q = mid.copy()
        q[a] = -1e300
        pts.append(q[None, :])
        q = mid.copy()
        q[a] = 1e300
        pts.append(q[None, :])
    # on faces (one coordinate a probe's), on edges (two), and a shade to either side of a face
    inner = pos[len(pos) // 2]
    for a in range(3):
        q = mid + 0.37 * step * 0.5
        q[a] = inner[a]
        pts.append(q[None, :])
        for eps in (-2.0 ** -40, 2.0 ** -40):
            r = q.copy()
            r[a] = inner[a] + eps
            pts.append(r[None, :])
        e = inner.copy()
        e[a] = mid[a] + 0.21 * step[a]
        pts.append(e[None, :])
    # Two runs of 64 entries, each starting at a multiple of 64 so that each is one wave of the kernel: the first inside ONE cell, an
    # interior one where the axis has one (index (N - 1) // 2: not 0 for N >= 3), with fractions of its own per lane -- the
    # wave-uniform path --; the second alternating between that cell and its neighbour on the first axis of at least 3 probes
    # (two real cells; a grid without such an axis cannot alternate) -- the gather path.
    head = np.concatenate(pts, axis=0)
    pad = (-len(head)) % 64
    filler = mid + 0.31 * step * np.linspace(-1.0, 1.0, pad)[:, None] if pad else np.zeros((0, 3))
    cell = np.array([(N - 1) // 2 if N >= 2 else 0 for N in grid.count], dtype=np.float64)
    t = (np.arange(64) + 0.5) / 64.0
    frac = np.stack([0.1 + 0.8 * t, 0.1 + 0.8 * t[::-1], 0.15 + 0.7 * ((7 * np.arange(64)) % 64 + 0.5) / 64.0], axis=1)
    one = lo + step * (cell[None, :] + frac)
    two = one.copy()
    wide = [a for a in range(3) if grid.count[a] >= 3]
    if wide:
        two[1::2, wide[0]] -= step[wide[0]]
    return np.concatenate([head, filler, one, two], axis=0)


def wave_runs(grid):
    """-> (index of the one-cell run's first entry, of the alternating run's): multiples of 64, for the tests that check the runs"""
    k = len(edge_points(grid)) - 128
    return k, k + 64


def entries(grid, m, seed=7):
    """m entries: the edge points first (as many as fit), random ones after them"""
    e = edge_points(grid)[:m]
    p, n = random_entries(grid, m, seed)
    p[:len(e)] = e
    return p, n

"""The restatement of the probe visibility (tests/probe_vis_expected.py) checked against itself on the CPU: its numpy form and its
scalar form agree bit for bit; the octahedral map's encoding inverts its texel centres; the lookup is continuous across the map's
edges and the z = 0 fold; moments that hide nothing reduce the extended shade to the plain one; the visibility weight stays in
[floor, 1]."""
import numpy as np
import pytest

import probe_expected as P
import probe_grid_expected as PG
import probe_vis_expected as PV

RES = (2, 3, 8, 32)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize])


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return ((_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))).all()


def _unit(rng, m):
    d = rng.normal(size=(m, 3))
    return d / np.linalg.norm(d, axis=1)[:, None]


# ---- 1. the two restatements agree ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", RES)
def test_texel_directions_agree(R):
    dirs = PV.texel_dirs(R)
    want = np.array([PV.texel_dir_scalar(R, i % R, i // R) for i in range(R * R)])
    assert (_bits(dirs) == _bits(want)).all()
    assert np.abs(np.linalg.norm(dirs, axis=1) - 1.0).max() < 2.0 ** -50
    # the lower half of the map is the lower hemisphere: z < 0 exactly where |a| + |b| > 1
    i = np.arange(R * R)
    a, b = ((i % R + 0.5) / R) * 2.0 - 1.0, ((i // R + 0.5) / R) * 2.0 - 1.0
    assert ((dirs[:, 2] < 0) == ((1.0 - np.abs(a)) - np.abs(b) < 0)).all()


@pytest.mark.parametrize("R", (2, 3, 8))
def test_lookups_agree(R):
    rng = np.random.default_rng(40 + R)
    maps = rng.normal(size=(4, R * R, 2))
    v = _unit(rng, 300) * rng.uniform(1e-3, 1e3, (300, 1))
    v[::11, 2] = 0.0
    v[5::13, 0] = 0.0
    v[7::17, :2] = 0.0
    v[9::19, 2] *= -1.0
    probe = rng.integers(0, 4, 300)
    mean, mean2 = PV.lookup(maps, probe, R, v)
    for k in range(300):
        m1, m2 = PV.lookup_scalar(maps[probe[k]], R, [float(x) for x in v[k]])
        assert _same(mean[k], np.float64(m1)) and _same(mean2[k], np.float64(m2)), (k, v[k])


@pytest.mark.parametrize("sharp", (0, 5, 8))
def test_folds_agree(sharp):
    rng = np.random.default_rng(50 + sharp)
    n, s = 3, 7
    vis = PV.Vis(res=3, sharp=sharp, d_max=2.5)
    rays = np.concatenate([rng.normal(size=(n * s, 3)), _unit(rng, n * s)], axis=1)
    status = rng.integers(0, 2, n * s).astype(np.uint32)
    status[s + 2] = 2                       # probe 1 is invalid
    t = rng.uniform(0.1, 5.0, n * s)       # on both sides of d_max
    sums, pst = PV.fold(rays, status, t, s, vis)
    assert list(pst) == [1, 2, 1] and np.isnan(sums[1]).all() and np.isfinite(sums[[0, 2]]).all()
    for probe in range(n):
        for texel in range(9):
            want = PV.fold_scalar(rays, status, t, s, vis, probe, texel % 3, texel // 3)
            assert _same(sums[probe, texel], np.array(want)), (probe, texel)
    mom = PV.resolve(sums, vis.d_max)
    for probe in range(n):
        for texel in range(9):
            assert _same(mom[probe, texel], np.array(PV.resolve_scalar(*[float(x) for x in sums[probe, texel]], vis.d_max)))
    # a texel no ray faces keeps d_max and its square
    empty = PV.resolve(np.zeros((1, 1, 3)), vis.d_max)
    assert (empty[0, 0] == [vis.d_max, vis.d_max * vis.d_max]).all()


@pytest.mark.parametrize("count", PG.COUNTS)
@pytest.mark.parametrize("flags", (0, PG.FACING))
def test_shades_agree(flags, count):
    grid = PG.Grid(count=count, flags=flags)
    vis = PV.Vis(step=grid.step, res=3)
    coeff, mom = PG.coefficients(grid), PV.random_moments(grid, vis)
    mom[0, 0] = np.nan
    m = 150
    p, n = PG.entries(grid, m)
    rng = np.random.default_rng(3)
    status = np.ones(m, dtype=np.uint32)
    status[5::17] = 0
    p[11::29, 1] = np.nan
    n[13::31, 2] = np.inf
    albedo, add = rng.random((m, 3)).astype(np.float32), rng.random((m, 3)).astype(np.float32)
    E, color = PV.shade_vis(grid, vis, coeff, mom, p, n, status, albedo, add)
    for k in range(m):
        e, c = PV.shade_vis_scalar(grid, vis, coeff, mom, p[k], n[k], status[k], albedo[k], add[k])
        assert _same(E[k], np.array(e)) and _same(color[k], np.array(c, dtype=np.float32)), (k, p[k], n[k])


# ---- 2. the map ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", RES)
def test_encoding_a_texel_centre_returns_it(R):
    """every texel of the map, so both halves of the z < 0 fold: the sample position of the centre direction (times any length: the
    encoding divides by the L1 norm) is the texel's own (tx, ty) to 2^-40 of a texel"""
    dirs = PV.texel_dirs(R)
    i = np.arange(R * R)
    for scale in (1.0, 3.7e-3, 1e6):
        ux, uy = PV.sample_position(R, dirs * scale)
        err = max(np.abs(ux - (i % R)).max(), np.abs(uy - (i // R)).max())
        assert err <= 2.0 ** -40, (R, scale, err)


def _largest_texel_step(maps, R):
    """the largest difference between a texel and a neighbour, the neighbours past an edge taken by the continuation"""
    i, j = np.meshgrid(np.arange(R), np.arange(R), indexing="xy")
    i, j = i.ravel(), j.ravel()
    here = maps[:, i + R * j]
    return max(np.abs(here - maps[:, PV._texel(R, i + di, j + dj)]).max() for di, dj in ((1, 0), (-1, 0), (0, 1), (0, -1)))


@pytest.mark.parametrize("R", RES)
def test_lookup_is_continuous_across_edges_and_the_fold(R):
    """Two unit directions delta = 2^-20 apart.  The unfolded coordinates a = v.x / s, s >= 1 the L1 norm, move by at most
    |dv.x| / s + |v.x| |ds| / s^2 <= delta + sqrt(3) delta < 3 delta; the fold's (1 - |b|) sgn(a) moves as b does, and where sgn(a)
    flips below z = 0 the two positions are the two sides of a map edge, which the continuation identifies.  A sample position moves
    by R / 2 per unit of a, so the path between the two positions, through an edge if one lies between, is at most 2 axes x (R / 2)
    x 3 delta texels long, and twice that if it is bent at an edge; the bilinear lookup changes by at most D a texel of path, D the
    largest texel-to-texel difference of the map.  Bound: 6 R delta D, and 2^-40 D for the roundings."""
    rng = np.random.default_rng(60 + R)
    maps = rng.normal(size=(1, R * R, 2))
    delta = 2.0 ** -20
    D = _largest_texel_step(maps, R)
    bound = 6.0 * R * delta * D + 2.0 ** -40 * D
    m = 400
    base = _unit(rng, m)
    kind = np.arange(m) % 4
    base[kind == 0, 2] = 0.0                                  # on the z = 0 fold: the map's inner diamond
    base[kind == 1, 0] = 0.0                                  # a = 0: below z = 0 the fold's sign flips, a map edge
    base[kind == 1, 2] = -np.abs(base[kind == 1, 2])
    base[kind == 2, 1] = 0.0                                  # b = 0 likewise
    base[kind == 2, 2] = -np.abs(base[kind == 2, 2])
    base[kind == 3, :2] = 0.0                                 # the poles: z = -1 is the map's four corners
    base[kind == 3, 2] = np.where(np.arange((kind == 3).sum()) % 2 == 0, -1.0, 1.0)
    base /= np.linalg.norm(base, axis=1)[:, None]
    step = _unit(rng, m) * (0.5 * delta)
    v1, v2 = base + step, base - step
    v1 /= np.linalg.norm(v1, axis=1)[:, None]
    v2 /= np.linalg.norm(v2, axis=1)[:, None]
    assert np.linalg.norm(v1 - v2, axis=1).max() <= delta * (1.0 + 2.0 ** -30)
    # the pairs do straddle: a sign of z, of x below z = 0, of y below z = 0 differs in most of them
    straddle = ((v1[:, 2] < 0) != (v2[:, 2] < 0)) | ((v1[:, 0] < 0) != (v2[:, 0] < 0)) | ((v1[:, 1] < 0) != (v2[:, 1] < 0))
    assert straddle.mean() > 0.6
    zero = np.zeros(m, dtype=np.int64)
    a1, a2 = PV.lookup(maps, zero, R, v1), PV.lookup(maps, zero, R, v2)
    worst = max(np.abs(a1[0] - a2[0]).max(), np.abs(a1[1] - a2[1]).max())
    print(f"R = {R}: largest difference {worst:.3e}, bound {bound:.3e}")
    assert worst <= bound


def test_edge_continuation_as_stated():
    R = 8
    assert PV._texel_scalar(R, -1, 3) == 0 + R * (R - 1 - 3)
    assert PV._texel_scalar(R, -1, -1) == (R - 1) + R * (R - 1)
    assert PV._texel_scalar(R, R, 2) == (R - 1) + R * (R - 1 - 2)
    assert PV._texel_scalar(R, 2, R) == (R - 1 - 2) + R * (R - 1)
    i, j = np.meshgrid(np.arange(-1, R + 1), np.arange(-1, R + 1))
    got = PV._texel(R, i.ravel(), j.ravel())
    want = [PV._texel_scalar(R, int(a), int(b)) for a, b in zip(i.ravel(), j.ravel())]
    assert (got == want).all() and got.min() >= 0 and got.max() < R * R


# ---- 3. the shade ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", PG.COUNTS)
@pytest.mark.parametrize("flags", (0, PG.FACING))
def test_moments_that_hide_nothing_give_the_plain_shade(flags, count):
    """mean >= r for every corner of every entry (the mean is 1e9; the entries lie within a few steps of the grid): vis_w = 1.0 and
    w_c * 1.0 = w_c, so every bit is probe_grid_expected's"""
    grid = PG.Grid(count=count, flags=flags)
    vis = PV.Vis(step=grid.step, res=4)
    coeff = PG.coefficients(grid)
    coeff[-1] = np.nan if grid.n > 1 else coeff[-1]
    mom = np.empty((grid.n, 16, 2))
    mom[..., 0], mom[..., 1] = 1e9, 1e18 + 5.0
    m = 400
    p, n = PG.entries(grid, m)
    finite = np.abs(p) < 1e200
    p = np.where(finite, p, 0.0)              # (the clamp tests at 1e300 are farther than any mean)
    status = np.ones(m, dtype=np.uint32)
    status[3::19] = 0
    add = np.random.default_rng(8).random((m, 3)).astype(np.float32)
    E, color = PV.shade_vis(grid, vis, coeff, mom, p, n, status, None, add)
    E0, color0 = PG.shade(grid, coeff, p, n, status, None, add)
    assert _same(E, E0) and _same(color, color0)


@pytest.mark.parametrize("flags", (0, PG.FACING))
def test_the_weight_stays_in_its_range(flags):
    grid = PG.Grid(count=(2, 3, 4), flags=flags)
    for floor in (2.0 ** -6, 0.5, 1.0):
        vis = PV.Vis(step=grid.step, res=8, floor=floor)
        mom = PV.random_moments(grid, vis)
        p, n = PG.random_entries(grid, 2000)
        E, _, w = PV.shade_vis(grid, vis, PG.coefficients(grid), mom, p, n, weights=True)
        counted = ~np.isnan(w)
        assert counted.any() and (w[counted] >= floor).all() and (w[counted] <= 1.0).all()
        assert (w[counted] < 1.0).any() or floor == 1.0
        assert np.isfinite(E).all()
    # r <= mean gives exactly 1: means at d_max beyond every distance
    mom[..., 0], mom[..., 1] = 1e6, 1e12
    _, _, w = PV.shade_vis(grid, vis, PG.coefficients(grid), mom, p, n, weights=True)
    assert (w[~np.isnan(w)] == 1.0).all()


def test_defaults_follow_the_grid():
    vis = PV.Vis(step=PG.STEP)
    sx, sy, sz = PG.STEP
    assert vis.res == 8 and vis.sharp == 5 and vis.floor == 2.0 ** -6
    assert vis.d_max == 1.5 * np.sqrt((sx * sx + sy * sy) + sz * sz) and vis.bias == 0.125 * min(PG.STEP)

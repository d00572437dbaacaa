"""Probe visibility on the GPU (include/rt_hip.h, "probe visibility"): the baked depth moments equal the restatement
(tests/probe_vis_expected.py) of the probe rays and the ray query's answers bit for bit, whatever the slices; the extended shade
equals its restatement bit for bit and, with moments that hide nothing, the plain shade; a wall between a lit and a dark room stops
leaking; the _vis preview is the stated composition of the public calls, in the device form, the host form, the host library and
the CLI; and every refusal leaves the outputs untouched."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest

import probe_expected as P
import probe_grid_expected as PG
import probe_vis_expected as PV

pytestmark = pytest.mark.gpu

DEPTH = 4
W, H = 33, 17
PREVIEW_COUNT, PREVIEW_SAMPLES = (4, 3, 4), 16
_CACHE = {}


@pytest.fixture
def gpu():
    import torch
    from rt_amd import abi, gpu as G
    assert abi.load_shim().rt_hip_device_count() >= 1, "no HIP device: the GPU tests must run on the GPU box"
    assert torch.cuda.is_available()
    return G


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32, 1: np.uint8}[a.dtype.itemsize])


def _host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _same(a, b):
    """bit-equal, a NaN matching any NaN"""
    return ((_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))).all()


def _dev(a, dtype=None):
    import torch
    a = np.ascontiguousarray(a)
    return torch.as_tensor(a if dtype is None else a.astype(dtype), device="cuda:0")


def _cube_scene():
    """config 1's spheres and the cube of tests/golden/c3_cube.obj, as tests/test_gpu_probe_grid.py sets it up, W x H"""
    import os
    from rt_amd import abi, scene as Sc
    host = abi.load_host()
    mesh = abi.TriangleMesh()
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "c3_cube.obj")
    assert host.load_obj(gold.encode(), C.byref(mesh))
    host.rt_mesh_flip_winding(C.byref(mesh))
    for k in range(36):
        v = mesh.vertices[k]
        v.pos = abi.Vec3(v.pos.x * 4, v.pos.y * 4 - 1, v.pos.z * 4)
    sc = Sc.build_scene(1, W, H, 1, DEPTH)
    meshes = (abi.MeshObject * 1)()
    meshes[0].flags = abi.M_REFLECTION
    meshes[0].color = abi.Vec3(0.9, 0.8, 0.7)
    meshes[0].emission = abi.Vec3(0, 0, 0)
    meshes[0].mesh = mesh
    sc.meshes, sc.n_meshes, sc.n_triangles = meshes, 1, 12
    return sc


def _quad(corner, e1, e2, facing):
    """two triangles of the parallelogram corner + s e1 + t e2 whose normal -- (v2 - v0) x (v1 - v0), the tracer's -- looks along
    `facing`"""
    c, e1, e2 = (np.asarray(x, dtype=np.float64) for x in (corner, e1, e2))
    a, b = (e1, e2) if np.dot(np.cross(e2, e1), facing) > 0 else (e2, e1)
    return [[c, c + a, c + b], [c + a, c + a + b, c + b]]


def _box(lo, hi, inward):
    """the six faces of a box, looking inward (a room) or outward (a slab)"""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    s = 1.0 if inward else -1.0
    d = hi - lo
    ex, ey, ez = np.array([d[0], 0, 0]), np.array([0, d[1], 0]), np.array([0, 0, d[2]])
    tris = []
    tris += _quad(lo, ey, ez, (s, 0, 0)) + _quad(lo + ex, ey, ez, (-s, 0, 0))
    tris += _quad(lo, ex, ez, (0, s, 0)) + _quad(lo + ey, ex, ez, (0, -s, 0))
    tris += _quad(lo, ex, ey, (0, 0, s)) + _quad(lo + ez, ex, ey, (0, 0, -s))
    return tris


WALL = dict(lo=(-4.0, 0.0, -2.0), hi=(4.0, 3.0, 2.0), half=0.1)


def _wall_scene():
    """Two rooms of triangles, x in [-4, -0.1] (dark) and [0.1, 4] (lit), y in [0, 3], z in [-2, 2], joined by a slab wall 0.2 thick,
    every face looking into its room; the lit room holds a sphere of radius 0.5 that emits 20"""
    from rt_amd import abi, scene as Sc
    lo, hi, h = WALL["lo"], WALL["hi"], WALL["half"]
    tris = _box(lo, (-h, hi[1], hi[2]), True) + _box((h, lo[1], lo[2]), hi, True)
    meshes = [dict(flags=abi.M_DEFAULT, color=(0.7, 0.7, 0.7), triangles=np.array(tris))]
    objs = [dict(flags=abi.M_DEFAULT, radius=0.5, center=(2.0, 2.2, 0.0), color=(0.0, 0.0, 0.0), emission=(20.0, 20.0, 20.0))]
    return Sc.custom_scene(objs, W, H, 1, DEPTH, (3.5, 1.5, 1.5), (0.0, 1.5, 0.0), meshes=meshes)


def _scene(gpu, name):
    if name not in _CACHE:
        from rt_amd import scene as Sc
        sc = {"room": lambda: Sc.build_scene(4, W, H, 1, DEPTH), "mesh": _cube_scene, "wall": _wall_scene}[name]()
        _CACHE[name] = (sc, gpu.GpuScene(sc))
    return _CACHE[name]


# ---- 1. the moments equal their restatement ------------------------------------------------------------------------------------------------
BAKE_GRID = PG.Grid(origin=(-2.0, 0.0, -2.0), step=(4.0, 2.0, 4.0), count=(2, 2, 2))
BAKE_SETS = {1: np.array([[0.5, 1.0, -0.5]]), 3: np.array([[0.5, 1.0, -0.5], [np.nan, 0.0, 0.0], [-2.0, 0.5, 1.5]]), 8: PG.positions(BAKE_GRID)}


def _restated_moments(gpu, gs, pos, s, vis):
    """gpu.probe_rays, GpuScene.query_rays, the numpy fold and resolve -> (moments, probe status)"""
    rays = gpu.probe_rays(pos, s, P.SEED)
    hits = gs.query_rays(rays, want=("status", "t"))
    sums, pst = PV.fold(_host(rays), _host(hits["status"]).view(np.uint32), _host(hits["t"]), s, vis)
    return PV.resolve(sums, vis.d_max), pst


@pytest.mark.parametrize("name", ["mesh", "room"])
@pytest.mark.parametrize("n", [1, 3, 8])
def test_moments_equal_the_restatement(gpu, name, n):
    sc, gs = _scene(gpu, name)
    pos = BAKE_SETS[n]
    cases = 0
    for s, R, sharp in itertools.product((1, 7, 64), (2, 3, 8), (0, 5)):
        vis = PV.Vis(res=R, sharp=sharp, d_max=3.0)
        want, want_status = _restated_moments(gpu, gs, pos, s, vis)
        where = BAKE_GRID.abi() if n == 8 else pos
        got = gs.probe_depth_moments(where, vis.abi(), s, P.SEED, details=True)
        mom, status = _host(got["moments"]), _host(got["status"]).view(np.uint32)
        assert mom.shape == want.shape == (n, R * R, 2)
        assert _same(mom, want), (s, R, sharp, np.argwhere(_bits(mom) != _bits(want))[:4])
        assert (status == want_status).all()
        if n == 3:   # the probe at a NaN position: its moments are NaN and its status 2, the others are untouched
            assert np.isnan(mom[1]).all() and list(status) == [1, 2, 1] and np.isfinite(mom[[0, 2]]).all()
        else:
            # (a mean of distances that are all d_max is d_max but for its roundings: at most 64 adds and a division, 2^-53 each)
            assert np.isfinite(mom).all() and (mom[..., 0] > 0).all() and (mom[..., 0] <= vis.d_max * (1.0 + 2.0 ** -46)).all()
        cases += 1
    print(f"{name}, N = {n}: {cases} bakes equal the restatement bit for bit")


@pytest.mark.parametrize("n,s", [(3, 7), (3, 64), (8, 7)])
def test_slices_change_no_bit(gpu, n, s):
    sc, gs = _scene(gpu, "room")
    vis = PV.Vis(res=3, sharp=5, d_max=3.0).abi()
    where = BAKE_GRID.abi() if n == 8 else BAKE_SETS[n]
    outs = []
    for slice_rays in (5, 64, n * s):   # 5 cuts a probe's rays
        got = gs.probe_depth_moments(where, vis, s, P.SEED, slice_rays=slice_rays, details=True)
        outs.append((_host(got["moments"]), _host(got["status"])))
    for mom, status in outs[1:]:
        assert _same(mom, outs[0][0]) and (status == outs[0][1]).all()


def test_the_depth_bake_shares_the_radiance_bake_rays(gpu):
    """bake_probe_grid(vis=...) returns the moments of rt_hip_bake_probe_grid_depth under the same samples and seed: those of
    probe_depth_moments at the grid's positions, and the coefficients are the plain bake's"""
    sc, gs = _scene(gpu, "room")
    vis = PV.Vis(step=BAKE_GRID.step, res=3)
    coeff, mom = gs.bake_probe_grid(BAKE_GRID.abi(), 7, P.SEED, max_depth=DEPTH, vis=vis.abi(BAKE_GRID.abi()))
    plain = gs.bake_probe_grid(BAKE_GRID.abi(), 7, P.SEED, max_depth=DEPTH)
    alone = gs.probe_depth_moments(PG.positions(BAKE_GRID), vis.abi(BAKE_GRID.abi()), 7, P.SEED)
    assert (_bits(_host(coeff)) == _bits(_host(plain))).all() and (_bits(_host(mom)) == _bits(_host(alone))).all()


# ---- 2. the shade ---------------------------------------------------------------------------------------------------------------------------
def _shade(gpu, grid, vis, coeff, mom, p, n, status=None, albedo=None, add=None, **kw):
    out = gpu.probe_shade(grid.abi(), _dev(coeff), _dev(p), _dev(n), None if status is None else _dev(status.view(np.int32)),
                          None if albedo is None else _dev(albedo), None if add is None else _dev(add),
                          vis=None if vis is None else vis.abi(grid.abi()), moments=None if vis is None else _dev(mom), **kw)
    return {k: _host(v) for k, v in out.items()}


def _inputs(grid, m):
    p, n = PG.entries(grid, m)
    rng = np.random.default_rng(100 + m)
    status = np.ones(m, dtype=np.uint32)
    if m > 8:
        status[5::17] = 0
        status[9::23] = 2
        p[11::29, 1] = np.nan
        n[13::31, 2] = np.inf
        p[14::37, 0] = -np.inf
        n[15::41, 0] = np.nan
    albedo = rng.random((m, 3)).astype(np.float32)
    add = (rng.random((m, 3)) * 2.0).astype(np.float32)
    return p, n, status, albedo, add


@pytest.mark.parametrize("count", PG.COUNTS)
@pytest.mark.parametrize("flags", (0, PG.FACING))
@pytest.mark.parametrize("m", (1, 63, 64, 65, 257, 1000))
def test_shade_equals_the_restatement(gpu, m, flags, count):
    """random moments on both sides of every r; m = 1000 holds PG.edge_points' run of 64 entries in one cell (the wave-uniform arm)
    and its alternating run (the gather arm)"""
    grid = PG.Grid(count=count, flags=flags)
    vis = PV.Vis(step=grid.step, res=(8, 3)[m % 2])
    coeff, mom = PG.coefficients(grid), PV.random_moments(grid, vis)
    p, n, status, albedo, add = _inputs(grid, m)
    if m == 1000:
        assert PG.wave_runs(grid)[1] + 64 <= m, "the two runs of 64 do not fit"
    for use in ((False, False, False), (True, False, True), (True, True, True)):
        st, al, ad = (x if u else None for x, u in zip((status, albedo, add), use))
        E, color = PV.shade_vis(grid, vis, coeff, mom, p, n, st, al, ad)
        got = _shade(gpu, grid, vis, coeff, mom, p, n, st, al, ad)
        assert _same(got["irradiance"], E), (use, np.argwhere(_bits(got["irradiance"]) != _bits(E))[:4])
        assert _same(got["color"], color), (use, np.argwhere(_bits(got["color"]) != _bits(color))[:4])
    E0, _ = PG.shade(grid, coeff, p, n, status, albedo, add)
    if m >= 257 and grid.n > 1:
        assert not _same(E, E0), "the moments change nothing: the test is blind"
    for want in (("irradiance",), ("color",)):
        alone = _shade(gpu, grid, vis, coeff, mom, p, n, status, albedo, add, want=want)
        assert list(alone) == list(want) and _same(alone[want[0]], got[want[0]])


@pytest.mark.parametrize("count", PG.COUNTS)
@pytest.mark.parametrize("flags", (0, PG.FACING))
def test_the_anchor(gpu, flags, count):
    """every mean is d_max, ten diagonals of the grid and more than any r of these entries: vis_w = 1.0 at every corner and the
    outputs are rt_hip_probe_shade's bit for bit"""
    grid = PG.Grid(count=count, flags=flags)
    diagonal = math.sqrt(sum(((c - 1) * s) ** 2 for c, s in zip(grid.count, grid.step))) + math.sqrt(sum(s * s for s in grid.step))
    vis = PV.Vis(step=grid.step, res=4, d_max=10.0 * diagonal)
    coeff = PG.coefficients(grid)
    mom = np.empty((grid.n, 16, 2))
    mom[..., 0], mom[..., 1] = vis.d_max, vis.d_max * vis.d_max
    p, n = PG.random_entries(grid, 1000)
    rng = np.random.default_rng(4)
    status = np.ones(1000, dtype=np.uint32)
    status[7::19] = 0
    albedo, add = rng.random((1000, 3)).astype(np.float32), rng.random((1000, 3)).astype(np.float32)
    got = _shade(gpu, grid, vis, coeff, mom, p, n, status, albedo, add)
    plain = _shade(gpu, grid, None, coeff, None, p, n, status, albedo, add)
    assert _same(got["irradiance"], plain["irradiance"]) and _same(got["color"], plain["color"])


def test_classes_and_their_neighbours(gpu):
    grid = PG.Grid(count=(2, 3, 4), flags=PG.FACING)
    vis = PV.Vis(step=grid.step, res=8)
    coeff, mom = PG.coefficients(grid), PV.random_moments(grid, vis)
    m = 200
    p, n = PG.random_entries(grid, m)
    add = np.random.default_rng(1).random((m, 3)).astype(np.float32)
    status = np.ones(m, dtype=np.uint32)
    clean = _shade(gpu, grid, vis, coeff, mom, p, n, status, None, add)
    bad_p, bad_n, miss = [10, 70, 130], [20, 80, 140], {30: 0, 90: 2, 150: 0xFFFFFFFF}
    p2, n2, st2 = p.copy(), n.copy(), status.copy()
    for i, v in zip(bad_p, (np.nan, np.inf, -np.inf)):
        p2[i, i % 3] = v
    for i, v in zip(bad_n, (np.nan, np.inf, -np.inf)):
        n2[i, i % 3] = v
    for i, v in miss.items():
        st2[i] = v
    got = _shade(gpu, grid, vis, coeff, mom, p2, n2, st2, None, add)
    touched = np.zeros(m, dtype=bool)
    touched[bad_p + bad_n + list(miss)] = True
    for f in ("irradiance", "color"):
        assert np.isnan(got[f][bad_p + bad_n]).all()
        assert (_bits(got[f][~touched]) == _bits(clean[f][~touched])).all()
    rows = list(miss)
    assert (_bits(got["irradiance"][rows]) == 0).all()
    want = (np.array(grid.miss_color)[None, :] + add[rows].astype(np.float64)).astype(np.float32)
    assert (_bits(got["color"][rows]) == _bits(want)).all()


def test_a_sub_range_writes_nothing_outside_itself(gpu):
    import torch
    grid = PG.Grid(count=(2, 3, 4))
    vis = PV.Vis(step=grid.step, res=3)
    coeff, mom = PG.coefficients(grid), PV.random_moments(grid, vis)
    total, first, m = 300, 64, 129
    p, n = PG.random_entries(grid, total)
    E, color = PV.shade_vis(grid, vis, coeff, mom, p, n)
    guard_d, guard_f = -7.25, np.float32(-3.5)
    irr = torch.full((total, 3), guard_d, dtype=torch.float64, device="cuda:0")
    col = torch.full((total, 3), float(guard_f), dtype=torch.float32, device="cuda:0")
    gpu.probe_shade(grid.abi(), _dev(coeff), _dev(p[first:]), _dev(n[first:]), out=dict(irradiance=irr[first:], color=col[first:]), m=m,
                    vis=vis.abi(grid.abi()), moments=_dev(mom))
    irr, col = _host(irr), _host(col)
    inside = np.zeros(total, dtype=bool)
    inside[first:first + m] = True
    assert (irr[~inside] == guard_d).all() and (col[~inside] == guard_f).all()
    assert (_bits(irr[inside]) == _bits(E[inside])).all() and (_bits(col[inside]) == _bits(color[inside])).all()


@pytest.mark.parametrize("flags", (0, PG.FACING))
def test_a_nan_moment_probe_counts_only_where_it_lights(gpu, flags):
    """the middle probe of a 3 x 3 x 3 grid has NaN moments and finite coefficients: entries where its weight is +0.0 -- the other
    probes' positions, the grid's outer faces -- are finite, entries strictly inside its cells are NaN (tests/test_gpu_probe_grid.py's
    construction, with the poison in the moments)"""
    grid = PG.Grid(origin=(-1.0, 0.0, 2.0), step=(0.5, 0.25, 1.0), count=(3, 3, 3), flags=flags)
    vis = PV.Vis(step=grid.step, res=3)
    coeff, mom = PG.coefficients(grid), PV.random_moments(grid, vis)
    poisoned = (1 * 3 + 1) * 3 + 1
    mom[poisoned] = np.nan
    pos = PG.positions(grid)
    step = np.array(grid.step)
    rng = np.random.default_rng(11)
    outer = pos[[i for i in range(27) if i != poisoned]]
    face = pos[0] + rng.random((96, 3)) * 2.0 * step
    axis, side = rng.integers(0, 3, 96), rng.integers(0, 2, 96)
    face[np.arange(96), axis] = np.where(side == 0, pos[0][axis], pos[26][axis])
    inside = pos[0] + (0.05 + 0.9 * rng.random((96, 3))) * 2.0 * step
    inside = inside[(np.abs(inside - pos[poisoned]) > 1e-6 * step).all(axis=1)]
    p = np.concatenate([outer, face, inside])
    n = rng.normal(size=p.shape)
    n /= np.linalg.norm(n, axis=1)[:, None]
    E, color = PV.shade_vis(grid, vis, coeff, mom, p, n)
    k = len(outer) + len(face)
    assert np.isfinite(E[:k]).all() and np.isnan(E[k:]).all()
    got = _shade(gpu, grid, vis, coeff, mom, p, n)
    assert np.isfinite(got["irradiance"][:k]).all() and np.isnan(got["irradiance"][k:]).all()
    assert _same(got["irradiance"], E) and _same(got["color"], color)


# ---- 3. the wall ----------------------------------------------------------------------------------------------------------------------------
WALL_SEED, WALL_SEED_B = 20261021, 20261022
WALL_PROBE_SAMPLES, WALL_REF_SAMPLES = 4096, 16384


def test_the_wall_stops_leaking(gpu):
    """Two rooms and a slab wall at x = 0 (_wall_scene), the emitter in the room at x > 0; a 4 x 4 x 2 grid over both, probes at
    x = -3, -1, 1, 3: the cell x in [-1, 1] straddles the wall.  4096 rays a probe, seed 20261021; the reference of an entry is
    bake_irradiance at it, 16384 paths, path traced.  FACING on both sides, rt_hip_probe_vis_defaults' parameters.
    Dark side: six points on the dark room's floor, ceiling, back walls and on the wall's own dark face, all in the straddling cell:
    the visibility-weighted irradiance is nearer the reference than the plain one, for every entry (compared on the channel sum: the
    scene is grey).
    Lit side: six points on the lit room's surfaces in the cell x in [1, 3], whose eight probes all stand in the lit room: E_vis stays
    within the reference's own sample spread of E_plain.  The spread: the reference is baked twice, seeds 20261021 and 20261022; the
    difference of two independent estimates of one mean has twice the variance of one, so the largest |E_a - E_b| over the six
    entries estimates about sqrt(2) x 1.6 standard errors (the expected largest of six half-normals); that number is taken as it
    stands, without a factor."""
    sc, gs = _scene(gpu, "wall")
    grid = PG.Grid(origin=(-3.0, 0.5, -1.0), step=(2.0, 2.0 / 3.0, 2.0), count=(4, 4, 2), flags=PG.FACING)
    g = grid.abi()
    from rt_amd import abi
    vis = abi.probe_vis(g)
    coeff, mom = gs.bake_probe_grid(g, WALL_PROBE_SAMPLES, WALL_SEED, max_depth=DEPTH, vis=vis)
    assert np.isfinite(_host(coeff)).all() and np.isfinite(_host(mom)).all()
    dark_p = np.array([[-0.5, 0.0, 0.6], [-0.7, 0.0, -0.8], [-0.4, 3.0, 0.3], [-0.6, 1.5, -2.0], [-0.5, 1.2, 2.0], [-0.1, 1.4, 0.2]])
    dark_n = np.array([[0, 1, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [-1, 0, 0]], dtype=np.float64)
    lit_p = np.array([[2.0, 0.0, 0.5], [1.5, 0.0, -0.7], [2.5, 3.0, 0.4], [2.0, 1.0, -2.0], [1.6, 1.8, 2.0], [2.4, 0.0, -0.2]])
    lit_n = np.array([[0, 1, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [0, 1, 0]], dtype=np.float64)
    p, n = np.concatenate([dark_p, lit_p]), np.concatenate([dark_n, lit_n])
    ref_a = _host(gs.bake_irradiance(p, n, WALL_REF_SAMPLES, WALL_SEED, bias=1e-6, max_depth=DEPTH)).sum(axis=1)
    ref_b = _host(gs.bake_irradiance(p, n, WALL_REF_SAMPLES, WALL_SEED_B, bias=1e-6, max_depth=DEPTH)).sum(axis=1)
    plain = _host(gpu.probe_shade(g, coeff, _dev(p), _dev(n), want=("irradiance",))["irradiance"]).sum(axis=1)
    seen = _host(gpu.probe_shade(g, coeff, _dev(p), _dev(n), want=("irradiance",), vis=vis, moments=mom)["irradiance"]).sum(axis=1)
    spread = np.abs(ref_a[6:] - ref_b[6:]).max()
    for k in range(12):
        print(f"{'dark' if k < 6 else 'lit '} {p[k]}: reference {ref_a[k]:.5f} / {ref_b[k]:.5f}, plain {plain[k]:.5f}, vis {seen[k]:.5f}")
    print(f"lit side: the reference's spread {spread:.5f}, largest |E_vis - E_plain| {np.abs(seen[6:] - plain[6:]).max():.5f}")
    assert (ref_a[6:] > 10.0 * ref_a[:6].max()).all(), "the dark room is not dark"
    assert (np.abs(seen[:6] - ref_a[:6]) < np.abs(plain[:6] - ref_a[:6])).all()
    assert (np.abs(seen[6:] - plain[6:]) <= spread).all()


# ---- 4. the preview is the stated composition ------------------------------------------------------------------------------------------------
def _preview_grid(flags=0):
    return PG.Grid(origin=(-6.0, -1.5, -6.0), step=(4.0, 2.5, 4.0), count=PREVIEW_COUNT, flags=flags)


def _emission_table(sc):
    rows = [sc.objects[i].emission.tuple() for i in range(sc.n_objects)] + [sc.meshes[k].emission.tuple() for k in range(sc.n_meshes)]
    return np.array(rows, dtype=np.float64).reshape(-1, 3)


def _composition(gpu, sc, gs, grid, vis, aov_samples, seed):
    """bake_probes and probe_depth_moments at probe_grid_positions; query_uv at the pixel centres; render_aov and its untile;
    probe_shade with the moments; the tonemap -> (coeff, moments, rgb float32 [H, W, 3], rgb8 uint8 [H, W, 3])"""
    import torch
    from rt_amd.gpu import n_tiles
    pos = gpu.probe_grid_positions(grid.abi())
    coeff = gs.bake_probes(pos, PREVIEW_SAMPLES, seed, max_depth=DEPTH)
    mom = gs.probe_depth_moments(pos, vis, PREVIEW_SAMPLES, seed)
    x, y = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    uv = np.stack([(x + 0.5) / (W - 1.0), (y + 0.5) / (H - 1.0)], axis=2).reshape(-1, 2)
    hits = gs.query_uv(uv, want=("status", "point", "normal", "object"))
    total = n_tiles(W, H)
    albedo = gs.untile_aov(gs.render_aov(seed, aov_samples, 0, 1, total, want=("albedo",)), 0, 1, total)["albedo"]
    obj = _host(hits["object"]).view(np.uint32)
    table = _emission_table(sc)
    add = np.zeros((W * H, 3), dtype=np.float32)
    hit = obj < len(table)
    add[hit] = table[obj[hit]].astype(np.float32)
    color = gpu.probe_shade(grid.abi(), coeff, hits["point"], hits["normal"], hits["status"], albedo.reshape(-1, 3), _dev(add), want=("color",),
                            vis=vis, moments=mom)["color"]
    rgb = color.reshape(H, W, 3)
    _, rgb8 = gpu.lens_resolve(rgb.to(torch.float64), 1)     # the render epilogue's tonemap of (double)rgb
    return _host(coeff), _host(mom), _host(rgb), _host(rgb8)


@pytest.mark.parametrize("name", ["room", "mesh"])
def test_preview_is_the_stated_composition(gpu, name):
    from rt_amd import abi
    sc, gs = _scene(gpu, name)
    for flags, aov_samples in ((0, 1), (PG.FACING, 3)):
        grid = _preview_grid(flags)
        vis = abi.probe_vis(grid.abi(), res=4)
        coeff, mom, rgb, rgb8 = _composition(gpu, sc, gs, grid, vis, aov_samples, P.SEED)
        assert np.isfinite(coeff).all() and np.isfinite(mom).all() and rgb8.std() > 0
        for slice_rays in (None, 1000):
            baked = gs.bake_probe_grid(grid.abi(), PREVIEW_SAMPLES, P.SEED, max_depth=DEPTH, slice_rays=slice_rays, details=True, vis=vis)
            assert (_bits(_host(baked["coeff"])) == _bits(coeff)).all() and (_bits(_host(baked["moments"])) == _bits(mom)).all()
            assert (_host(baked["depth_status"]) == 1).all()
            got, got8 = gs.probe_preview(grid.abi(), baked["coeff"], aov_samples=aov_samples, seed=P.SEED, vis=vis, moments=baked["moments"])
            got, got8 = _host(got), _host(got8)
            assert _same(got, rgb), np.argwhere(_bits(got) != _bits(rgb))[:4]
            assert (got8 == rgb8).all()
        # the host form, and the plain preview when vis is absent
        h_rgb, h_rgb8, h_coeff, h_mom, stats = gpu.probe_preview_vis_host(sc, grid.abi(), vis, PREVIEW_SAMPLES, P.SEED, aov_samples=aov_samples,
                                                                          max_depth=DEPTH)
        assert (_bits(h_coeff) == _bits(coeff)).all() and (_bits(h_mom) == _bits(mom)).all()
        assert _same(h_rgb, rgb) and (h_rgb8 == rgb8).all() and stats["samples"] == grid.n * PREVIEW_SAMPLES
        plain, plain8 = gs.probe_preview(grid.abi(), _dev(coeff), aov_samples=aov_samples, seed=P.SEED)
        p_rgb, p_rgb8, _, _ = gpu.probe_preview_host(sc, grid.abi(), PREVIEW_SAMPLES, P.SEED, aov_samples=aov_samples, max_depth=DEPTH)
        assert _same(_host(plain), p_rgb) and (_host(plain8) == p_rgb8).all()


def _grid_over_the_scene(gs, count):
    """rt_set_probe_grid's grid (include/raytracer.h): [-reach, reach] an axis about the world's origin"""
    from rt_amd import abi
    reach = C.c_double()
    assert gs.shim.rt_hip_scene_bounds(gs.handle, None, None, C.byref(reach), None) == 0
    r = reach.value if reach.value > 0 else 1.0
    return abi.probe_grid([-r if n >= 2 else 0.0 for n in count], [(2.0 * r) / float(n - 1) if n >= 2 else 1.0 for n in count], count)


def test_cli_takes_a_fourth_number(gpu, tmp_path):
    """raytracer -m 4,4,4,4: the PNG's bytes are the _vis host form's for the grid over the scene's bounds and the defaults at R = 4;
    -m 4,4,4: the plain preview's"""
    import os
    import subprocess
    import util
    from rt_amd import abi
    cli = os.path.join(os.path.dirname(abi.HOST_PATH), "raytracer")
    sc, gs = _scene(gpu, "room")
    grid = _grid_over_the_scene(gs, (4, 4, 4))
    frames = {}
    for arg in ("4,4,4,4", "4,4,4"):
        png = str(tmp_path / f"preview_{len(arg)}.png")
        r = subprocess.run([cli, "-c", "4", "-w", str(W), "-h", str(H), "-s", str(PREVIEW_SAMPLES), "-d", str(DEPTH), "-r", str(P.SEED), "-m", arg,
                            "-o", png], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        frames[arg] = np.asarray(util.decode_png_rgb8(png)).reshape(H, W, 3)
    _, want8, _, _, _ = gpu.probe_preview_vis_host(sc, grid, abi.probe_vis(grid, res=4), PREVIEW_SAMPLES, P.SEED, aov_samples=1, max_depth=DEPTH)
    _, plain8, _, _ = gpu.probe_preview_host(sc, grid, PREVIEW_SAMPLES, P.SEED, aov_samples=1, max_depth=DEPTH)
    assert (frames["4,4,4,4"] == want8).all() and (frames["4,4,4"] == plain8).all() and want8.std() > 0
    for bad in ("4,4,4,", "4,4,4,1", "4,4,4,33", "4,4,4,x", "4,4,4,4,4"):
        r = subprocess.run([cli, "-c", "4", "-w", str(W), "-h", str(H), "-s", "4", "-m", bad, "-o", str(tmp_path / "bad.png")], capture_output=True,
                           text=True, timeout=60)
        assert r.returncode != 0 and "Usage" in r.stderr, bad


def test_host_library_setter(gpu):
    """rt_set_probe_visibility(res) turns render()'s probe-lit preview into the _vis one; 0 restores the plain frame, bit for bit"""
    from rt_amd import abi
    host = abi.load_host()
    sc, gs = _scene(gpu, "room")
    assert host.rt_get_probe_visibility() == 0
    for bad in (1, 33, -4):
        host.rt_set_probe_visibility(bad)
        assert host.rt_get_probe_visibility() == 0
    grid = _grid_over_the_scene(gs, (4, 4, 4))
    opt = abi.Options()
    opt.width, opt.height, opt.samples = W, H, PREVIEW_SAMPLES
    depth0, seed0 = host.rt_get_max_depth(), host.rt_get_seed()
    host.rt_set_max_depth(DEPTH)
    host.rt_set_seed(P.SEED)
    host.rt_set_probe_grid(4, 4, 4)
    frames = []
    try:
        for res in (0, 4, 0):
            host.rt_set_probe_visibility(res)
            assert host.rt_get_probe_visibility() == res
            fb, lin = np.zeros((H, W, 3), dtype=np.uint8), np.zeros((H, W, 3), dtype=np.float32)
            host.render_ex(fb.ctypes.data, lin.ctypes.data, sc.objects, sc.n_objects, sc.meshes if sc.n_meshes else None, sc.n_meshes,
                           C.byref(sc.camera), C.byref(opt))
            frames.append(fb)
    finally:
        host.rt_set_probe_visibility(0)
        host.rt_set_probe_grid(0, 0, 0)
        host.rt_set_max_depth(depth0)
        host.rt_set_seed(seed0)
    _, want8, _, _, _ = gpu.probe_preview_vis_host(sc, grid, abi.probe_vis(grid, res=4), PREVIEW_SAMPLES, P.SEED, aov_samples=1, max_depth=DEPTH)
    _, plain8, _, _ = gpu.probe_preview_host(sc, grid, PREVIEW_SAMPLES, P.SEED, aov_samples=1, max_depth=DEPTH)
    assert (frames[0] == plain8).all() and (frames[1] == want8).all() and (frames[2] == plain8).all()


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched(gpu):
    import torch
    from rt_amd import abi
    shim = abi.load_shim()
    sc, gs = _scene(gpu, "room")
    grid = PG.Grid(count=(2, 3, 4))
    g = grid.abi()
    good = abi.probe_vis(g, res=3)
    pp = abi.probe_params(abi.PROBE_SPHERE, 4, P.SEED, DEPTH, 0.0, 10.0)
    n = grid.n
    pos = _dev(PG.positions(grid))
    ws = torch.zeros(shim.rt_hip_probe_depth_workspace_bytes(n, 32, n * 4) + 64, dtype=torch.uint8, device="cuda:0")
    mom = torch.full((n, 32 * 32, 2), -7.25, dtype=torch.float64, device="cuda:0")
    status = torch.full((n,), 77, dtype=torch.int32, device="cuda:0")
    coeff = _dev(PG.coefficients(grid))
    p, nrm = PG.random_entries(grid, 64)
    p, nrm = _dev(p), _dev(nrm)
    irr = torch.full((64, 3), -7.25, dtype=torch.float64, device="cuda:0")
    ptr = lambda t: C.c_void_p(t.data_ptr())

    def bake(vis, params=pp, scene=gs.handle, positions=pos, work=ws, out=mom, count=n, slice_rays=1000):
        return shim.rt_hip_bake_probe_depth(scene, None if positions is None else ptr(positions), count, None if vis is None else C.byref(vis),
                                            C.byref(params), slice_rays, None if work is None else ptr(work), None if out is None else ptr(out),
                                            ptr(status), None)

    def shade(vis, moments=mom):
        return shim.rt_hip_probe_shade_vis(C.byref(g), None if vis is None else C.byref(vis), ptr(coeff), None if moments is None else ptr(moments),
                                           ptr(p), ptr(nrm), None, None, None, 64, ptr(irr), None, None)

    def changed(**fields):
        v = abi.probe_vis(g, res=3)
        for f, x in fields.items():
            setattr(v, f, x)
        return v

    bad = [changed(res=1), changed(res=33), changed(res=0), changed(sharp=9), changed(d_max=0.0), changed(d_max=-1.0),
           changed(d_max=float("inf")), changed(d_max=float("nan")), changed(bias=-1e-9), changed(bias=float("inf")),
           changed(bias=float("nan")), changed(floor=0.0), changed(floor=1.0 + 2.0 ** -52), changed(floor=float("nan")),
           changed(floor=-0.5), changed(reserved=1), changed(flags=1), changed(struct_size=40)]
    for v in bad:
        assert bake(v) == abi.EINVAL and shade(v) == abi.EINVAL, (v.res, v.sharp, v.d_max, v.bias, v.floor, v.reserved, v.flags)
    assert bake(None) == abi.EINVAL and shade(None) == abi.EINVAL
    # N * R * R above 2^28 (the positions are not read: the refusal comes before any launch)
    assert bake(changed(res=32), count=(1 << 18) + 1) == abi.EINVAL
    assert shim.rt_hip_probe_depth_workspace_bytes((1 << 18) + 1, 32, 64) == 0 and shim.rt_hip_probe_depth_workspace_bytes(1 << 18, 32, 64) > 0
    # a misaligned workspace, NULL required pointers, a hemisphere bake, no slice
    assert shim.rt_hip_bake_probe_depth(gs.handle, ptr(pos), n, C.byref(good), C.byref(pp), 1000, C.c_void_p(ws.data_ptr() + 8), ptr(mom),
                                        ptr(status), None) == abi.EINVAL
    assert bake(good, scene=None) == abi.EINVAL and bake(good, positions=None) == abi.EINVAL and bake(good, work=None) == abi.EINVAL
    assert bake(good, out=None) == abi.EINVAL and bake(good, slice_rays=0) == abi.EINVAL and shade(good, moments=None) == abi.EINVAL
    assert bake(good, params=abi.probe_params(abi.PROBE_HEMISPHERE, 4, P.SEED, DEPTH, 0.0, 10.0)) == abi.EINVAL
    # the grid form and the preview refuse the same vis
    gws = torch.zeros(shim.rt_hip_probe_grid_depth_workspace_bytes(C.byref(g), 3, 1000) + 64, dtype=torch.uint8, device="cuda:0")
    assert shim.rt_hip_bake_probe_grid_depth(gs.handle, C.byref(g), C.byref(bad[0]), C.byref(pp), 1000, ptr(gws), ptr(mom), ptr(status), None) == abi.EINVAL
    assert shim.rt_hip_bake_probe_grid_depth(gs.handle, C.byref(g), C.byref(good), C.byref(pp), 1000, ptr(gws), None, ptr(status), None) == abi.EINVAL
    pws = torch.zeros(shim.rt_hip_probe_preview_workspace_bytes(gs.handle, W, H), dtype=torch.uint8, device="cuda:0")
    rgb = torch.full((H, W, 3), -3.5, dtype=torch.float32, device="cuda:0")
    for v, m in ((bad[3], mom), (good, None)):
        assert shim.rt_hip_probe_preview_vis(gs.handle, C.byref(sc.camera), C.byref(g), C.byref(v), ptr(coeff), None if m is None else ptr(m), W, H,
                                             1, 0, ptr(pws), ptr(rgb), None, None) == abi.EINVAL
    torch.cuda.synchronize()
    assert (_host(mom) == -7.25).all() and (_host(status) == 77).all() and (_host(irr) == -7.25).all() and (_host(rgb) == -3.5).all()
    # and the good arguments are taken
    assert bake(good) == 0 and shade(good) == 0
    assert bake(good, count=0, positions=None, work=None, out=None) == 0
    torch.cuda.synchronize()
    assert (_host(status) == 1).all() and np.isfinite(_host(irr)).all()


def test_zz_close(gpu):
    for sc, gs in _CACHE.values():
        gs.close()
        sc.free()
    _CACHE.clear()

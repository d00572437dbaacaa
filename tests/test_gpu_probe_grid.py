"""Probe grids on the GPU (include/rt_hip.h, "probe grids"): the grid's positions and the shade equal the restatement
(tests/probe_grid_expected.py) bit for bit over every output, entry class and optional input; a NaN probe outside an entry's support
does not reach it; constant and affine fields come back; and the preview is the stated composition of the calls that exist, in the
device form and the host form."""
import ctypes as C
import itertools

import numpy as np
import pytest

import probe_expected as P
import probe_grid_expected as PG

pytestmark = pytest.mark.gpu

DEPTH = 4
W, H = 32, 24
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
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda:0") if dtype is None else torch.as_tensor(np.ascontiguousarray(a).astype(dtype), device="cuda:0")


def _shade(gpu, grid, coeff, p, n, status=None, albedo=None, add=None, **kw):
    out = gpu.probe_shade(grid.abi(), _dev(coeff), _dev(p), _dev(n), None if status is None else _dev(status.view(np.int32)),
                          None if albedo is None else _dev(albedo), None if add is None else _dev(add), **kw)
    return {k: _host(v) for k, v in out.items()}


# ---- 1. the positions ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", PG.COUNTS)
def test_positions_equal_the_restatement(gpu, count):
    grid = PG.Grid(count=count)
    got = _host(gpu.probe_grid_positions(grid.abi()))
    want = PG.positions(grid)
    assert got.shape == want.shape and (_bits(got) == _bits(want)).all()


# ---- 2. the shade, bit for bit --------------------------------------------------------------------------------------------------------------
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
    grid = PG.Grid(count=count, flags=flags)
    coeff = PG.coefficients(grid)
    p, n, status, albedo, add = _inputs(grid, m)
    for use in itertools.product((False, True), repeat=3):
        st, al, ad = (x if u else None for x, u in zip((status, albedo, add), use))
        E, color = PG.shade(grid, coeff, p, n, st, al, ad)
        got = _shade(gpu, grid, coeff, p, n, st, al, ad)
        assert _same(got["irradiance"], E), (use, np.argwhere(_bits(got["irradiance"]) != _bits(E))[:4])
        assert _same(got["color"], color), (use, np.argwhere(_bits(got["color"]) != _bits(color))[:4])
    # either output alone is the same output
    for want in (("irradiance",), ("color",)):
        alone = _shade(gpu, grid, coeff, p, n, status, albedo, add, want=want)
        assert list(alone) == list(want) and _same(alone[want[0]], got[want[0]])


# ---- 3. the classes ---------------------------------------------------------------------------------------------------------------------
def test_classes_and_their_neighbours(gpu):
    grid = PG.Grid(count=(2, 3, 4), flags=PG.FACING)
    coeff = PG.coefficients(grid)
    m = 200
    p, n = PG.random_entries(grid, m)
    add = np.random.default_rng(1).random((m, 3)).astype(np.float32)
    status = np.ones(m, dtype=np.uint32)
    clean = _shade(gpu, grid, coeff, p, n, status, None, add)
    bad_p, bad_n, miss = [10, 70, 130], [20, 80, 140], {30: 0, 90: 2, 150: 0xFFFFFFFF}
    p2, n2, st2 = p.copy(), n.copy(), status.copy()
    for i, v in zip(bad_p, (np.nan, np.inf, -np.inf)):
        p2[i, i % 3] = v
    for i, v in zip(bad_n, (np.nan, np.inf, -np.inf)):
        n2[i, i % 3] = v
    for i, v in miss.items():
        st2[i] = v
    got = _shade(gpu, grid, coeff, p2, n2, st2, None, add)
    touched = np.zeros(m, dtype=bool)
    touched[bad_p + bad_n + list(miss)] = True
    for f in ("irradiance", "color"):
        assert np.isnan(got[f][bad_p + bad_n]).all()
        assert (_bits(got[f][~touched]) == _bits(clean[f][~touched])).all()
    rows = list(miss)
    assert (_bits(got["irradiance"][rows]) == 0).all()
    want = (np.array(grid.miss_color)[None, :] + add[rows].astype(np.float64)).astype(np.float32)
    assert (_bits(got["color"][rows]) == _bits(want)).all()
    # a NaN point under a status word that is not 1 is a miss, not an invalid entry
    st2[bad_p[0]] = 0
    again = _shade(gpu, grid, coeff, p2, n2, st2, None, add)
    assert (_bits(again["irradiance"][bad_p[0]]) == 0).all()


def test_a_sub_range_writes_nothing_outside_itself(gpu):
    import torch
    grid = PG.Grid(count=(2, 3, 4))
    coeff = PG.coefficients(grid)
    total, first, m = 300, 64, 129
    p, n = PG.random_entries(grid, total)
    E, color = PG.shade(grid, coeff, p, n)
    guard_d, guard_f = -7.25, np.float32(-3.5)
    irr = torch.full((total, 3), guard_d, dtype=torch.float64, device="cuda:0")
    col = torch.full((total, 3), float(guard_f), dtype=torch.float32, device="cuda:0")
    gpu.probe_shade(grid.abi(), _dev(coeff), _dev(p[first:]), _dev(n[first:]), out=dict(irradiance=irr[first:], color=col[first:]), m=m)
    irr, col = _host(irr), _host(col)
    inside = np.zeros(total, dtype=bool)
    inside[first:first + m] = True
    assert (irr[~inside] == guard_d).all() and (col[~inside] == guard_f).all()
    assert (_bits(irr[inside]) == _bits(E[inside])).all() and (_bits(col[inside]) == _bits(color[inside])).all()


# ---- 4. corners of weight zero are skipped --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", (0, PG.FACING))
def test_a_nan_probe_outside_the_support(gpu, flags):
    # origin and steps are powers of two, so that a point on a face has an integer g exactly
    grid = PG.Grid(origin=(-1.0, 0.0, 2.0), step=(0.5, 0.25, 1.0), count=(3, 3, 3), flags=flags)
    coeff = PG.coefficients(grid)
    poisoned = (1 * 3 + 1) * 3 + 1    # the middle probe: it borders all eight cells
    coeff[poisoned] = np.nan
    pos = PG.positions(grid)
    step = np.array(grid.step)
    rng = np.random.default_rng(11)
    # at the other probes, and on the outer faces of the grid -- faces of cells it borders --, its weight is +0.0
    outer = pos[[i for i in range(27) if i != poisoned]]
    face = pos[0] + rng.random((96, 3)) * 2.0 * step
    axis = rng.integers(0, 3, 96)
    side = rng.integers(0, 2, 96)
    face[np.arange(96), axis] = np.where(side == 0, pos[0][axis], pos[26][axis])
    # strictly inside its cells: every entry there has it in its support
    inside = pos[0] + (0.05 + 0.9 * rng.random((96, 3))) * 2.0 * step
    inside = inside[(np.abs(inside - pos[poisoned]) > 1e-6 * step).all(axis=1)]
    p = np.concatenate([outer, face, inside])
    n = rng.normal(size=p.shape)
    n /= np.linalg.norm(n, axis=1)[:, None]
    E, color = PG.shade(grid, coeff, p, n)
    k = len(outer) + len(face)
    assert np.isfinite(E[:k]).all() and np.isnan(E[k:]).all()
    got = _shade(gpu, grid, coeff, p, n)
    assert np.isfinite(got["irradiance"][:k]).all() and np.isnan(got["irradiance"][k:]).all()
    assert _same(got["irradiance"], E) and _same(got["color"], color)


# ---- 5. what a blend must give back -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", (0, PG.FACING))
def test_partition_of_unity(gpu, flags):
    """every probe holds the same coefficients: the blend is those coefficients but for its roundings -- 8 products added and divided
    by their weight sum, about 20 roundings of 2^-53 over nine bases: a relative 2^-46 of rt_hip_probe_irradiance for that probe.
    Channels the restatement clamps at 0 are left out, by its own sign."""
    grid = PG.Grid(count=(2, 3, 4), flags=flags)
    one = np.random.default_rng(21).normal(0.0, 1.0, (9, 3))
    one[0] = np.abs(one[0]) + 6.0     # a field that is mostly positive
    coeff = np.broadcast_to(one, (grid.n, 9, 3)).copy()
    p, n = PG.random_entries(grid, 1000, seed=22)
    n = np.random.default_rng(23).normal(size=n.shape)
    n /= np.linalg.norm(n, axis=1)[:, None]
    got = _shade(gpu, grid, coeff, p, n, want=("irradiance",))["irradiance"]
    want = _host(gpu.probe_irradiance(_dev(coeff[:1]), np.zeros(1000, dtype=np.int64), _dev(n)))
    E, _ = PG.shade(grid, coeff, p, n)
    keep = (E > 0.0) & (want > 0.0)
    assert keep.mean() > 0.9
    rel = np.abs(got[keep] - want[keep]) / np.abs(want[keep])
    print("partition of unity: largest relative error 2^%.2f" % np.log2(max(rel.max(), 2.0 ** -60)))
    assert (rel <= 2.0 ** -46).all()


def test_linear_field(gpu):
    """only basis 0 is non-zero and it is an affine function of the probe's position, no facing weight, points inside the grid:
    trilinear blending gives affine functions back, E = A_0 * Y0 * affine(p) to a relative 2^-44 (the bar covers the roundings of the
    cell's fractions and of the eight products)"""
    grid = PG.Grid(count=(4, 3, 5))
    pos = PG.positions(grid)
    a0, a = np.array([40.0, 50.0, 60.0]), np.array([[1.0, 0.5, 0.25], [0.3, 0.7, 0.2], [0.6, 0.1, 0.9]])   # [channel, axis]
    coeff = np.zeros((grid.n, 9, 3))
    coeff[:, 0, :] = a0[None, :] + pos @ a.T
    rng = np.random.default_rng(31)
    p = pos[0] + rng.random((1000, 3)) * (pos[-1] - pos[0])
    n = rng.normal(size=p.shape)
    n /= np.linalg.norm(n, axis=1)[:, None]
    got = _shade(gpu, grid, coeff, p, n, want=("irradiance",))["irradiance"]
    want = P.A[0] * P.Y0 * (a0[None, :] + p @ a.T)
    rel = np.abs(got - want) / np.abs(want)
    print("linear field: largest relative error 2^%.2f" % np.log2(max(rel.max(), 2.0 ** -60)))
    assert (rel <= 2.0 ** -44).all()


# ---- 6. the preview is the stated composition ---------------------------------------------------------------------------------------------------
def _cube_scene():
    """config 1's spheres and the cube of tests/golden/c3_cube.obj, as tests/test_gpu_probe.py sets it up, W x H"""
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


def _scene(gpu, name):
    if name not in _CACHE:
        from rt_amd import scene as Sc
        sc = {"room": lambda: Sc.build_scene(4, W, H, 1, DEPTH), "mesh": _cube_scene}[name]()
        _CACHE[name] = (sc, gpu.GpuScene(sc))
    return _CACHE[name]


def _preview_grid(flags=0):
    return PG.Grid(origin=(-6.0, -1.5, -6.0), step=(4.0, 2.5, 4.0), count=PREVIEW_COUNT, flags=flags)


def _emission_table(sc):
    rows = [sc.objects[i].emission.tuple() for i in range(sc.n_objects)] + [sc.meshes[k].emission.tuple() for k in range(sc.n_meshes)]
    return np.array(rows, dtype=np.float64).reshape(-1, 3)


def _composition(gpu, sc, gs, grid, aov_samples, seed):
    """bake_probes at probe_grid_positions; query_uv at the pixel centres; render_aov and its untile; probe_shade; the tonemap
    -> (coeff, rgb float32 [H, W, 3], rgb8 uint8 [H, W, 3], status, object)"""
    import torch
    from rt_amd.gpu import n_tiles
    pos = gpu.probe_grid_positions(grid.abi())
    coeff = gs.bake_probes(pos, PREVIEW_SAMPLES, seed, max_depth=DEPTH)
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
    color = gpu.probe_shade(grid.abi(), coeff, hits["point"], hits["normal"], hits["status"], albedo.reshape(-1, 3), _dev(add), want=("color",))["color"]
    rgb = color.reshape(H, W, 3)
    _, rgb8 = gpu.lens_resolve(rgb.to(torch.float64), 1)     # sum * (1.0 / 1.0) is the sum: the render epilogue's tonemap of (double)rgb
    return _host(coeff), _host(rgb), _host(rgb8), _host(hits["status"]).view(np.uint32), obj


@pytest.mark.parametrize("name", ["room", "mesh"])
def test_preview_is_the_stated_composition(gpu, name):
    sc, gs = _scene(gpu, name)
    for flags, aov_samples in ((0, 1), (PG.FACING, 3)):
        grid = _preview_grid(flags)
        coeff, rgb, rgb8, status, obj = _composition(gpu, sc, gs, grid, aov_samples, P.SEED)
        assert np.isfinite(coeff).all() and (status == 1).any()
        for slice_rays in (None, 1000):
            baked = gs.bake_probe_grid(grid.abi(), PREVIEW_SAMPLES, P.SEED, max_depth=DEPTH, slice_rays=slice_rays, details=True)
            assert (_bits(_host(baked["coeff"])) == _bits(coeff)).all() and (_host(baked["status"]) == 1).all()
            got, got8 = gs.probe_preview(grid.abi(), baked["coeff"], aov_samples=aov_samples, seed=P.SEED)
            got, got8 = _host(got), _host(got8)
            assert _same(got, rgb), np.argwhere(_bits(got) != _bits(rgb))[:4]
            assert (got8 == rgb8).all()
        assert np.isfinite(rgb[status.reshape(H, W) == 1]).all() and rgb8.std() > 0


def test_a_visible_emitter_shows_its_emission(gpu):
    sc, gs = _scene(gpu, "room")
    grid = _preview_grid()
    coeff, rgb, rgb8, status, obj = _composition(gpu, sc, gs, grid, 1, P.SEED)
    table = _emission_table(sc)
    lit = np.array([o < len(table) and table[o].max() > 0 for o in obj])
    assert lit.any(), "the room's light is not in view"
    flat = rgb.reshape(-1, 3)
    assert (flat[lit] >= table[obj[lit]].astype(np.float32)).all()
    got, _ = gs.probe_preview(grid.abi(), _dev(coeff), aov_samples=1, seed=P.SEED)
    assert (_host(got).reshape(-1, 3)[lit] >= table[obj[lit]].astype(np.float32)).all()


def test_host_form_on_a_logical_device(gpu):
    from rt_amd import abi
    shim = abi.load_shim()
    sc, gs = _scene(gpu, "room")
    grid = _preview_grid(PG.FACING)
    coeff, rgb, rgb8, _, _ = _composition(gpu, sc, gs, grid, 2, P.SEED)
    assert shim.rt_hip_set_device_map((C.c_int * 2)(0, 0), 2) == 0
    try:
        got, got8, got_coeff, stats = gpu.probe_preview_host(sc, grid.abi(), PREVIEW_SAMPLES, P.SEED, aov_samples=2, max_depth=DEPTH, device=1)
        with pytest.raises(gpu.ShimError):
            gpu.probe_preview_host(sc, grid.abi(), PREVIEW_SAMPLES, P.SEED, aov_samples=2, max_depth=DEPTH, device=2)
    finally:
        assert shim.rt_hip_set_device_map(None, 0) == 0
    assert (_bits(got_coeff) == _bits(coeff)).all()
    assert _same(got, rgb) and (got8 == rgb8).all()
    assert stats["samples"] == grid.n * PREVIEW_SAMPLES


def _grid_over_the_scene(gs, count):
    """rt_set_probe_grid's grid (include/raytracer.h): [-reach, reach] an axis about the world's origin"""
    from rt_amd import abi
    reach = C.c_double()
    assert gs.shim.rt_hip_scene_bounds(gs.handle, None, None, C.byref(reach), None) == 0
    r = reach.value if reach.value > 0 else 1.0
    return abi.probe_grid([-r if n >= 2 else 0.0 for n in count], [(2.0 * r) / float(n - 1) if n >= 2 else 1.0 for n in count], count)


def test_cli_writes_the_preview(gpu, tmp_path):
    """raytracer -m nx,ny,nz: the PNG's decoded bytes are the host form's for the grid over the scene's bounds, -s rays a probe"""
    import os
    import subprocess
    import util
    from rt_amd import abi, scene as Sc
    cli = os.path.join(os.path.dirname(abi.HOST_PATH), "raytracer")
    png = str(tmp_path / "preview.png")
    r = subprocess.run([cli, "-c", "4", "-w", str(W), "-h", str(H), "-s", str(PREVIEW_SAMPLES), "-d", str(DEPTH), "-r", str(P.SEED), "-m",
                        ",".join(str(n) for n in PREVIEW_COUNT), "-o", png], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = util.decode_png_rgb8(png)
    sc, gs = _scene(gpu, "room")
    grid = _grid_over_the_scene(gs, PREVIEW_COUNT)
    _, want8, coeff, stats = gpu.probe_preview_host(sc, grid, PREVIEW_SAMPLES, P.SEED, aov_samples=1, max_depth=DEPTH)
    assert np.asarray(got).reshape(H, W, 3).shape == want8.shape and (np.asarray(got).reshape(H, W, 3) == want8).all()
    assert np.isfinite(coeff).all() and want8.std() > 0
    for bad in ("4,3", "4,3,x", "0,3,4", "4,3,4,1", "4097,4096,2"):
        r = subprocess.run([cli, "-c", "4", "-w", str(W), "-h", str(H), "-s", "4", "-m", bad, "-o", png], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "Usage" in r.stderr, bad
    r = subprocess.run([cli, "-c", "4", "-w", str(W), "-h", str(H), "-s", "4", "-m", "2,2,2", "-p", "2", "-o", png], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode != 0 and "Usage" in r.stderr


def test_host_library_setter(gpu):
    from rt_amd import abi
    host = abi.load_host()
    nx, ny, nz = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    host.rt_get_probe_grid(C.byref(nx), C.byref(ny), C.byref(nz))
    assert (nx.value, ny.value, nz.value) == (0, 0, 0)
    host.rt_set_probe_grid(4, 3, 4)
    host.rt_get_probe_grid(C.byref(nx), C.byref(ny), C.byref(nz))
    assert (nx.value, ny.value, nz.value) == (4, 3, 4)
    host.rt_set_probe_grid(4, 0, 4)
    host.rt_get_probe_grid(C.byref(nx), C.byref(ny), C.byref(nz))
    assert (nx.value, ny.value, nz.value) == (0, 0, 0)


def test_zz_close(gpu):
    for sc, gs in _CACHE.values():
        gs.close()
        sc.free()
    _CACHE.clear()

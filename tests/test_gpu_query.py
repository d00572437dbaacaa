"""Ray queries on the GPU (rt_hip_query_*): for rays the caller chooses, status, t, object, primitive, point, normal, barycentrics and
the ray itself equal the CPU expectation built from the compiled reference (tests/query_expected.py) BIT FOR BIT -- one scene per
form of the query kernels, coincident triangles, walls, a lopsided hierarchy; every ray count around a wave and a workgroup; camera
(u, v) rays; normalisation over 600 binades; the band's edges; NaN and infinities in every slot; t_max at, above and below the
winner; origins on surfaces and far beyond near_R; tangent and in-plane rays; the origin_radius hint; permutations; the entry
point for C hosts and the host library's intersect_rays.  The last test checks that every form was launched under a comparison."""
import ctypes as C
import math

import numpy as np
import pytest

import query_expected as Q
import util

pytestmark = pytest.mark.gpu

COMPARED = set()   # query forms launched by a test of this module that compared their answers


@pytest.fixture
def gpu():
    import torch
    from rt_amd import abi, gpu as G
    assert abi.load_shim().rt_hip_device_count() >= 1, "no HIP device: the GPU tests must run on the GPU box"
    assert torch.cuda.is_available()
    return G


def _np(out):
    import torch
    torch.cuda.synchronize()
    res = {f: t.cpu().numpy() for f, t in out.items()}
    return {f: (a.view(np.uint32) if a.dtype == np.int32 else a) for f, a in res.items()}


def _check(gs, got, exp, what, fields=Q.FIELDS):
    msg = Q.mismatch(got, exp, fields)
    assert not msg, f"{what}: {msg}"
    assert gs.launch_status() == 0
    COMPARED.add(gs.query_kernel_name())


_CACHE = {}


def _scene(gpu, ref, name):
    """the scene, its GpuScene, its ray set and the reference's answers: computed once, shared, never changed"""
    if name not in _CACHE:
        sc = Q.SCENES[name][1]()
        rays = Q.ray_set(sc)
        _CACHE[name] = (sc, gpu.GpuScene(sc), rays, Q.expected(ref, sc, rays=rays))
    return _CACHE[name]


def _reach(sc):
    objs, meshes = util.scene_parts(sc)
    r = [np.linalg.norm(o["center"]) + o["radius"] for o in objs if o["radius"] < 1000]
    r += [np.sqrt((m["vertices"][:, :3] ** 2).sum(axis=1)).max() for m in meshes]
    return float(max(r))


@pytest.mark.parametrize("name", sorted(Q.SCENES))
def test_every_form_equals_the_reference(gpu, ref_mesh, name):
    sc, gs, rays, exp = _scene(gpu, ref_mesh(5), name)
    if Q.SCENES[name][0]:
        assert gs.query_kernel_name() == Q.SCENES[name][0]
    _check(gs, _np(gs.query_rays(rays)), exp, name)


@pytest.mark.parametrize("name", ["rays", "tri_big"])
def test_ray_counts_around_a_wave_and_a_workgroup(gpu, ref_mesh, name):
    sc, gs, rays, exp = _scene(gpu, ref_mesh(5), name)
    for n in (1, 63, 64, 65, 255, 256, 257):
        _check(gs, _np(gs.query_rays(rays[:n])), {f: a[:n] for f, a in exp.items()}, f"{name} n={n}")
    out = _np(gs.query_rays(rays[:0]))
    assert all(len(a) == 0 for a in out.values())


def test_each_output_may_be_left_out(gpu, ref_mesh):
    sc, gs, rays, exp = _scene(gpu, ref_mesh(5), "tri")
    for skip in Q.FIELDS:
        want = tuple(f for f in Q.FIELDS if f != skip)
        _check(gs, _np(gs.query_rays(rays[:300], want=want)), {f: a[:300] for f, a in exp.items()}, f"without {skip}", want)
    with pytest.raises(gpu.ShimError):
        gs.query_rays(rays[:4], want=())


@pytest.mark.parametrize("name,variant", [("tri", "sheared"), ("tri_big", "near_plane")])
def test_camera_uv_rays(gpu, ref_mesh, name, variant):
    base = Q.SCENES[name][1]()
    sc = util.view_variant(base, variant)
    rng = np.random.default_rng(5)
    uv = np.concatenate([rng.uniform(0, 1, (900, 2)), rng.uniform(-0.5, 1.5, (124, 2)), [[0.0, 0.0], [1.0, 1.0], [-3.0, 7.0]]])
    gs = gpu.GpuScene(sc)
    exp = Q.expected(ref_mesh(5), sc, uv=uv)
    assert (exp["status"] == 1).sum() > 100
    _check(gs, _np(gs.query_uv(uv)), exp, f"uv {name} {variant}")
    x, y = 17, 9
    one = Q.expected(ref_mesh(5), sc, uv=[[(x + 0.5) / (sc.width - 1), (y + 0.5) / (sc.height - 1)]])
    p = gs.pick(x, y)
    assert (p["status"], p["object"], p["prim"], p["t"]) == (one["status"][0], one["object"][0], one["prim"][0], one["t"][0])
    assert p["point"] == tuple(one["point"][0]) and p["normal"] == tuple(one["normal"][0])
    gs.close()


def test_normalize_over_six_hundred_binades(gpu, ref_mesh):
    sc, gs, rays, _ = _scene(gpu, ref_mesh(5), "tri")
    r = rays[:1024].copy()
    scale = 2.0 ** np.linspace(-300, 300, len(r)).round()
    r[:, 3:] *= scale[:, None]
    r[5, 3:] = 0.0                      # zero: 0 * inf, invalid
    r[6, 3:] *= 2.0 ** 600 / scale[6]   # the dot overflows: d * (1 / inf) = 0, invalid
    r[7, 3:] *= 2.0 ** -600 / scale[7]  # the dot underflows to 0: d * inf, invalid
    exp = Q.expected(ref_mesh(5), sc, rays=r, normalize_dirs=True)
    assert exp["status"][5] == 2 and exp["status"][6] == 2 and exp["status"][7] == 2 and (exp["status"] != 2).sum() == len(r) - 3
    got = _np(gs.query_rays(r, normalize=True))
    bad = exp["status"] == 2            # (a NaN's sign and payload are no part of the contract: compare the rest)
    for f in ("ray",):
        assert np.isnan(got[f][5, 3:]).all() and (got[f][6, 3:] == 0).all()
        got[f][bad], exp[f][bad] = 0.0, 0.0
    _check(gs, got, exp, "normalize")


def test_band_edges_without_normalize(gpu, ref_mesh):
    sc, gs, rays, _ = _scene(gpu, ref_mesh(5), "tri_big")
    r = rays[:512].copy()
    s = np.sqrt(1.0 + np.array([0.999, 1.001, -0.999, -1.001, 1e-6, -1e-6, 2.0 ** -39, 0.5])[np.arange(len(r)) % 8] * Q.BAND)
    r[:, 3:] *= s[:, None]
    exp = Q.expected(ref_mesh(5), sc, rays=r)
    assert 100 < (exp["status"] == 2).sum() < 160 and (exp["status"] == 1).sum() > 80
    _check(gs, _np(gs.query_rays(r)), exp, "band edges")


def test_non_finite_values_in_every_slot(gpu, ref_mesh):
    sc, gs, rays, exp0 = _scene(gpu, ref_mesh(5), "rays")
    r, t_max = rays[:256].copy(), np.full(256, np.finfo(np.float64).max)
    k = 3
    for slot in range(6):
        for bad in (math.nan, math.inf, -math.inf):
            r[k, slot] = bad
            k += 5
    t_max[200], t_max[201], t_max[202] = math.nan, math.inf, -math.inf
    exp = Q.expected(ref_mesh(5), sc, rays=r, t_max=t_max)
    assert (exp["status"] == 2).sum() == 19 and exp["status"][201] == exp0["status"][201] and exp["status"][202] == 0
    untouched = np.isfinite(r).all(axis=1) & (np.arange(256) < 200)
    assert (exp["t"][untouched] == exp0["t"][:256][untouched]).all()
    got = _np(gs.query_rays(r, t_max=t_max))
    assert (np.isnan(got["ray"]) == np.isnan(exp["ray"])).all()
    got["ray"][np.isnan(got["ray"])] = 0.0
    exp["ray"][np.isnan(exp["ray"])] = 0.0
    _check(gs, got, exp, "non-finite")


def test_t_max_at_above_and_below_the_winner(gpu, ref_mesh):
    sc, gs, rays, exp0 = _scene(gpu, ref_mesh(5), "soup")
    hit = np.nonzero(exp0["status"] == 1)[0][:500]
    r, t = rays[hit], exp0["t"][hit]
    cases = [t, np.nextafter(t, np.inf), np.nextafter(t, 0.0), np.zeros_like(t), -t, np.full_like(t, np.inf), np.full_like(t, 1e-8)]
    for k, t_max in enumerate(cases):
        exp = Q.expected(ref_mesh(5), sc, rays=r, t_max=t_max)
        assert (exp["status"] == 1).sum() == (len(hit) if k in (1, 5) else 0)
        _check(gs, _np(gs.query_rays(r, t_max=t_max)), exp, f"t_max case {k}")


@pytest.mark.parametrize("name", ["rays", "tri", "lopsided"])
def test_origins_on_surfaces_and_far_beyond_near_R(gpu, ref_mesh, name):
    sc, gs, rays, exp0 = _scene(gpu, ref_mesh(5), name)
    hit = np.nonzero(exp0["status"] == 1)[0][:600]
    d, n = rays[hit, 3:], exp0["normal"][hit]
    refl = Q.normalize(d - 2.0 * (d * n).sum(axis=1)[:, None] * n)
    on_surface = np.concatenate([exp0["point"][hit], refl], axis=1)
    near_R = 1.5 * _reach(sc) + 1.0
    far = rays[:600].copy()
    far[:300, :3] -= far[:300, 3:] * 10.0 * near_R       # back along the ray: the same primitives lie ahead
    far[300:, :3] -= far[300:, 3:] * 1e6 * near_R
    for what, r in (("on a surface", on_surface), ("far origins", far)):
        exp = Q.expected(ref_mesh(5), sc, rays=r)
        assert (exp["status"] != 2).all() and (exp["status"] == 1).sum() > 50
        _check(gs, _np(gs.query_rays(r)), exp, f"{name} {what}")


def test_tangent_rays_in_plane_rays_and_identical_spheres(gpu, ref_mesh):
    from rt_amd import abi, scene as S
    objs = [dict(flags=abi.M_DEFAULT, radius=2.0, center=(0.0, 0.0, 0.0), color=(1, 0, 0)),
            dict(flags=abi.M_DEFAULT, radius=2.0, center=(0.0, 0.0, 0.0), color=(0, 1, 0)),
            dict(flags=abi.M_DEFAULT, radius=1.5, center=(6.0, 1.0, -2.0), color=(0, 0, 1))]
    tri = [[(-3.0, -1.0, 5.0), (3.0, -1.0, 5.0), (0.0, 4.0, 5.0)], [(-3.0, -1.0, 5.0), (3.0, -1.0, 5.0), (0.0, 4.0, 5.0)],
           [(4.0, 0.0, 0.0), (9.0, 0.0, 0.0), (4.0, 0.0, 6.0)]]
    sc = S.custom_scene(objs, 32, 32, 1, 5, (0, 0, 20), (0, 0, 0), meshes=[dict(flags=abi.M_DEFAULT, color=(1, 1, 1), triangles=tri)])
    rng = np.random.default_rng(9)
    rays = []
    for k in range(200):   # tangent to the twin spheres: origin on the plane x = 2 (+- a few ulps), direction in that plane
        a = rng.uniform(0, 2 * np.pi)
        x = np.nextafter(2.0, [0.0, 4.0, 2.0][k % 3]) if k % 3 != 2 else 2.0
        rays.append([x, -8.0 * np.cos(a), -8.0 * np.sin(a), 0.0, np.cos(a), np.sin(a)])
    for k in range(200):   # in the plane y = 0 of the third triangle, and in the plane z = 5 of the coincident pair
        a = rng.uniform(0, 2 * np.pi)
        rays.append([6.0 - 9.0 * np.cos(a), 0.0, 2.0 - 9.0 * np.sin(a), np.cos(a), 0.0, np.sin(a)] if k % 2 else
                    [-9.0 * np.cos(a), 1.0 - 9.0 * np.sin(a), 5.0, np.cos(a), np.sin(a), 0.0])
    for k in range(200):   # through everything: the twin spheres (the lower index wins), the coincident triangles (the lower index wins)
        o = np.array([rng.uniform(-1, 1), rng.uniform(-0.5, 1.5), 12.0 if k % 2 else -12.0])
        rays.append(list(o) + [0.0, 0.0, -1.0 if k % 2 else 1.0])
    rays = np.array(rays)
    exp = Q.expected(ref_mesh(5), sc, rays=rays)
    thru = exp["status"][400:] == 1
    assert thru.all() and set(exp["object"][400:].tolist()) <= {0, 3} and set(exp["prim"][400:].tolist()) == {0, Q.NO_HIT}
    gs = gpu.GpuScene(sc)
    _check(gs, _np(gs.query_rays(rays)), exp, "tangent / in-plane / twins")
    gs.close()


@pytest.mark.parametrize("name", ["rays", "tri", "tri_big", "mem"])
def test_origin_radius_changes_no_bit_and_permutations_permute(gpu, ref_mesh, name):
    sc, gs, rays, exp = _scene(gpu, ref_mesh(5), name)
    for radius in (0.0, None, 100.0 * _reach(sc)):
        _check(gs, _np(gs.query_rays(rays, origin_radius=radius)), exp, f"{name} origin_radius {radius}")
    perm = np.random.default_rng(1).permutation(len(rays))
    _check(gs, _np(gs.query_rays(rays[perm])), {f: a[perm] for f, a in exp.items()}, f"{name} permuted")


def test_host_entry_points(gpu, ref_mesh):
    from rt_amd import abi
    sc, gs, rays, exp = _scene(gpu, ref_mesh(5), "tri")
    shim = abi.load_shim()
    assert shim.rt_hip_set_device_map((C.c_int * 3)(0, 0, 0), 3) == 0
    try:
        got = gpu.query_rays_host(sc, rays[:700], device=2)
        msg = Q.mismatch(got, {f: a[:700] for f, a in exp.items()})
        assert not msg, msg
        with pytest.raises(gpu.ShimError):
            gpu.query_rays_host(sc, rays[:4], device=3)
        cam_exp = Q.expected(ref_mesh(5), sc, uv=[[0.3, 0.6], [0.5, 0.5]])
        assert not Q.mismatch(gpu.query_rays_host(sc, [[0.3, 0.6], [0.5, 0.5]], camera=sc.camera, device=1), cam_exp)
    finally:
        assert shim.rt_hip_set_device_map(None, 0) == 0
    COMPARED.add(gs.query_kernel_name())
    # the host library: the reference's own Hit, u and v the winner's
    host = abi.load_host()
    n = 700
    extra = {}
    t_max = np.where(np.arange(n) % 7 == 0, exp["t"][:n], np.finfo(np.float64).max)
    e = Q.expected(ref_mesh(5), sc, rays=rays[:n], t_max=t_max, extra=extra)
    r = np.ascontiguousarray(rays[:n])
    hits, status = (abi.Hit * n)(), np.zeros(n, np.uint8)
    assert host.intersect_rays(C.cast(r.ctypes.data, C.POINTER(abi.Ray)), n, t_max.ctypes.data, sc.objects, sc.n_objects, sc.meshes, sc.n_meshes,
                               hits, status.ctypes.data) == 0
    assert (status == e["status"]).all()
    kinds = set()
    for i in range(n):
        h = hits[i]
        if e["status"][i] == 1:
            assert (h.t, h.object_id, h.point.tuple(), h.normal.tuple()) == (e["t"][i], e["object"][i], tuple(e["point"][i]), tuple(e["normal"][i]))
            assert (h.u, h.v) == (extra["u_win"][i], extra["v_win"][i]), (i, e["prim"][i])
            kinds.add(e["prim"][i] == Q.NO_HIT)
        else:
            assert h.t == np.finfo(np.float64).max and h.object_id == Q.NO_HIT and h.point.tuple() == (0, 0, 0)
    assert kinds == {True, False}


def test_zz_every_query_form_was_compared(gpu):
    from rt_amd import abi
    shim = abi.load_shim()
    for k in range(shim.rt_hip_query_kernel_count()):
        n = C.c_uint64(0)
        name = shim.rt_hip_query_kernel_launches(k, C.byref(n)).decode()
        assert n.value > 0 and name in COMPARED, f"{name}: {n.value} launches, compared: {name in COMPARED}"
    for sc, gs, _, _ in _CACHE.values():
        gs.close()
        sc.free()
    _CACHE.clear()

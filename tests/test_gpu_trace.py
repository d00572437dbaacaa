"""Radiance queries on the GPU (rt_hip_trace_*): for rays the caller chooses, the per-ray path and scan counters equal the compiled
reference exactly, every sample's value equals the reference's to 2^-40 relative, and the contract's four bit-exact statements hold --
one scene per form of the radiance-query kernels, config 3's cube and config 5's mesh, a glass and a checker room; ray counts around
the 64-ray workgroup, ragged sample slices, depth 4 and 8, stream indices up to 2^32; invalid, band, far, inside and on-surface rays;
the host form on a logical device; the tie to the renderer's own frames; the panorama.

The value bar.  The device's iteration (Ls += T e; T = T albedo cos) and the reference's recursion evaluate the same non-negative terms
e_j prod(albedo cos [/ p]) with at most about 5 (D + 2) roundings each, so they differ by at most 10 (D + 2) 2^-53 of the value:
2e-14 at D = 16; 2^-40 leaves 45 x room.  With M_REFRACTION the weights change sign: there the bar is 2^-40 (|ref| + the largest |ref|
among that ray's samples)."""
import ctypes as C

import numpy as np
import pytest

import trace_expected as T
import util

pytestmark = pytest.mark.gpu

COMPARED = set()
WORST = {}     # scene -> the worst observed |got - ref| / bar
_CACHE = {}


@pytest.fixture
def gpu():
    import torch
    from rt_amd import abi, gpu as G
    assert abi.load_shim().rt_hip_device_count() >= 1, "no HIP device: the GPU tests must run on the GPU box"
    assert torch.cuda.is_available()
    return G


ALL = ("status", "radiance", "samples", "paths", "casts", "ray")


def _np(out):
    import torch
    torch.cuda.synchronize()
    res = {f: t.cpu().numpy() for f, t in out.items()}
    res["status"] = res["status"].view(np.uint32) if "status" in res else None
    for f in ("paths", "casts"):
        if f in res:
            res[f] = res[f].view(np.uint64)
    return res


def _stats(a):
    return dict(rays=int(a[0]), casts=int(a[1]), tests=int(a[2]), samples=int(a[3]))


def _scene(gpu, name, depth):
    key = (name, depth)
    if key not in _CACHE:
        sc = T.SCENES[name][1](depth)
        _CACHE[key] = (sc, gpu.GpuScene(sc), T.ray_set(sc, open_back=name in T.OPEN_BACK))
    return _CACHE[key]


def _reach(sc):
    """the scene's extent as the launch's near_R = 1.5 (origin_radius + reach) + 1 takes it: spheres of ordinary size and vertices"""
    objs, meshes = util.scene_parts(sc)
    r = [np.linalg.norm(ob["center"]) + ob["radius"] for ob in objs if ob["radius"] < 1000]
    r += [np.sqrt((m["vertices"][:, :3] ** 2).sum(axis=1)).max() for m in meshes]
    return float(max(r))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _compare(gs, sc, name, got, ref, S, n, glass):
    assert (got["status"] == 1).all()
    assert (got["paths"] == ref["paths"]).all(), f"{name}: paths differ at rays {np.nonzero(got['paths'] != ref['paths'])[0][:5]}"
    assert (got["casts"] == ref["casts"]).all(), f"{name}: casts differ at rays {np.nonzero(got['casts'] != ref['casts'])[0][:5]}"
    st = _stats(got["stats"])
    assert st == dict(rays=int(ref["paths"].sum()), casts=int(ref["casts"].sum()), tests=int(ref["casts"].sum()) * sc.n_primitives,
                      samples=n * S), (name, st)
    err, bar = np.abs(got["samples"] - ref["samples"]), T.value_bar(ref["samples"], glass)
    ratio = float((err[bar > 0] / bar[bar > 0]).max()) if (bar > 0).any() else 0.0
    WORST[name] = max(WORST.get(name, 0.0), ratio)
    print(f"{name}: n={n} S={S} worst |got - ref| / bar = {ratio:.3e}")
    assert (err <= bar).all(), f"{name}: {(err > bar).sum()} sample values beyond the bar, worst ratio {ratio}"
    assert (_bits(got["radiance"]) == _bits(T.reduce_samples(got["samples"]))).all(), f"{name}: (a) radiance is not the reduction"
    assert (_bits(got["ray"]) == _bits(ref["rays"])).all()
    assert gs.launch_status() == 0
    COMPARED.add(gs.trace_kernel_name())


CASES = [("rays", 4, 257, 5, 0), ("rays", 8, 65, 9, 1000), ("big", 4, 64, 3, 0), ("tri", 8, 63, 4, 0), ("tri_big", 4, 65, 1, 1000),
         ("mem", 4, 64, 3, 0), ("glass", 4, 257, 5, 0), ("glass", 8, 65, 4, 2 ** 32 - 65), ("chk", 8, 64, 9, 0), ("cube", 4, 65, 3, 0),
         ("mesh", 4, 63, 1, 0), ("rays", 4, 1, 4, 2 ** 32 - 1)]


@pytest.mark.parametrize("name,depth,n,S,first", CASES)
def test_counters_and_values_equal_the_reference(gpu, ref_mesh, pt, name, depth, n, S, first):
    sc, gs, (o, q) = _scene(gpu, name, depth)
    assert gs.trace_kernel_name() == T.SCENES[name][0]
    ref = T.reference_samples(ref_mesh(depth), sc, o[:n], q[:n], S, T.SEED, first, casts_oracle=pt)
    got = _np(gs.trace_rays(ref["rays"], S, T.SEED, index_first=first, want=ALL))
    _compare(gs, sc, name, got, ref, S, n, T.SCENES[name][2])


@pytest.mark.parametrize("name", ["rays", "glass", "tri_big"])
def test_split_batches_sample_counts_and_query_rays_agree_bit_for_bit(gpu, name):
    sc, gs, (o, q) = _scene(gpu, name, 4)
    rays = np.concatenate([o, o - q], axis=1)
    rays[:, 3:] = T.Q.normalize(rays[:, 3:])
    whole = _np(gs.trace_rays(rays, 9, T.SEED, want=ALL))
    for a, b in ((0, 64), (64, 65), (65, 257)):                                          # (b) pieces under index_first
        part = _np(gs.trace_rays(rays[a:b], 9, T.SEED, index_first=a, want=ALL))
        for f in ALL:
            assert (part[f] == whole[f][a:b]).all() if f in ("status", "paths", "casts") else (_bits(part[f]) == _bits(whole[f][a:b])).all(), (name, f, a)
    four = _np(gs.trace_rays(rays, 4, T.SEED, want=ALL))                                 # (d) samples do not depend on S
    assert (_bits(four["samples"]) == _bits(whole["samples"][:, :4])).all()
    import torch
    q_ray = gs.query_rays(rays, want=("ray",))["ray"]                                    # (c) GIVEN
    torch.cuda.synchronize()
    assert (_bits(q_ray.cpu().numpy()) == _bits(whole["ray"])).all()
    scaled = rays.copy()
    scaled[:, 3:] *= np.linspace(0.25, 7.0, len(rays))[:, None]                          # (c) NORMALIZE
    t = _np(gs.trace_rays(scaled, 1, T.SEED, normalize=True, want=("status", "ray")))
    qn = gs.query_rays(scaled, normalize=True, want=("ray",))["ray"].cpu().numpy()
    assert (_bits(t["ray"]) == _bits(qn)).all() and (t["status"] == 1).all()
    uv = np.random.default_rng(4).uniform(-0.2, 1.2, (130, 2))                           # (c) CAMERA_UV
    t = _np(gs.trace_uv(uv, 3, T.SEED, want=ALL))
    qu = gs.query_uv(uv, want=("ray",))["ray"].cpu().numpy()
    assert (_bits(t["ray"]) == _bits(qu)).all()
    again = _np(gs.trace_rays(qu, 3, T.SEED, want=ALL))                                  # the same rays GIVEN: the same samples
    assert (_bits(again["samples"]) == _bits(t["samples"])).all()
    assert gs.launch_status() == 0


def test_edge_rays(gpu, ref_mesh, pt):
    sc, gs, (o, q) = _scene(gpu, "tri", 4)
    base = T.reference_samples(ref_mesh(4), sc, o[:8], q[:8], 1, T.SEED)["rays"]
    bad = base.copy()
    bad[0, 1] = np.nan                                  # a NaN origin
    bad[1, 3:] = 0.0                                    # a zero direction without NORMALIZE
    bad[2, 3:] *= np.sqrt(1.0 + 2.0 ** -12)             # |d|^2 = 1 + 2^-12
    got = _np(gs.trace_rays(bad, 5, T.SEED, want=ALL))
    assert got["status"].tolist() == [2, 2, 2, 1, 1, 1, 1, 1]
    for f in ("radiance", "samples", "paths", "casts"):
        assert (got[f][:3] == 0).all(), f
    assert np.isnan(got["ray"][0, 1]) and (_bits(got["ray"][1:]) == _bits(bad[1:])).all()
    assert _stats(got["stats"])["samples"] == 5 * 5
    # far origins, an origin inside a sphere and one exactly on a surface: the reference as given
    objs, _ = util.scene_parts(sc)
    small = [ob for ob in objs if ob["radius"] < 1000][0]
    c, r = np.array(small["center"]), small["radius"]
    n = 48
    o2, d2 = o[:n].copy(), T.Q.normalize(o[:n] - q[:n])
    o2[40:44] = c + 0.3 * r * d2[40:44]                 # inside a sphere
    o2[44:48] = c + r * d2[44:48]                       # on its surface, leaving along the normal
    near_R = 1.5 * _reach(sc) + 1.0                    # the launch's own, at origin_radius 0 (rt_hip.h)
    o2[32:40] = o2[32:40] - d2[32:40] * 10.0 * near_R   # beyond near_R: the same primitives lie ahead
    assert (np.sqrt((o2[32:40] ** 2).sum(axis=1)) > near_R).all()
    ref = T.reference_samples(ref_mesh(4), sc, o2, o2 - d2, 3, T.SEED, casts_oracle=pt)
    got = _np(gs.trace_rays(ref["rays"], 3, T.SEED, want=ALL))
    _compare(gs, sc, "tri", got, ref, 3, n, False)
    assert gs.launch_status() == 0


@pytest.mark.parametrize("name", ["rays", "tri", "tri_big"])
def test_band_rays_equal_the_reference_as_given(gpu, ref_mesh, pt, name):
    """|d|^2 = 1 +- 2^-14: valid, and scanned with no_rules.  No camera forms such a ray (get_camera_ray normalises), so the
    expectation is the reference's own scan of the ray as given and trace_path written out at MAX_DEPTH = 0
    (trace_expected.depth0_expected: bit for bit the oracle's samples on unit rays, tests/test_trace_cpu.py): paths and casts of
    every ray exactly, a miss's and a roulette death's value bit for bit, a bounce's to the bar"""
    sc, gs, (o, q) = _scene(gpu, name, 0)
    d = T.Q.normalize(o[:64] - q[:64])
    if name == "tri_big":                                # the room's back is open: rays that leave through it hit nothing
        d[48:64] = T.Q.normalize(np.array([0.0, 0.0, -1.0]) + 0.05 * (d[48:64] - d[48:64].mean(axis=0)))
    rays = np.concatenate([o[:64], d], axis=1)
    rays[0:64:2, 3:] *= np.sqrt(1.0 + 2.0 ** -14)
    rays[1:64:2, 3:] *= np.sqrt(1.0 - 2.0 ** -14)
    dd = (rays[:, 3] * rays[:, 3] + rays[:, 4] * rays[:, 4]) + rays[:, 5] * rays[:, 5]
    assert ((np.abs(dd - 1.0) > 2.0 ** -40) & (np.abs(dd - 1.0) <= 2.0 ** -13)).all()
    exp = T.depth0_expected(ref_mesh(4), pt, sc, rays, 3, T.SEED, 7)
    if name == "tri_big":
        assert 4 <= (~exp["hit"]).sum() <= 60
    assert exp["exact"].sum() >= 8 and (~exp["exact"]).sum() >= 64
    got = _np(gs.trace_rays(rays, 3, T.SEED, max_depth=0, index_first=7, want=ALL))
    assert (got["status"] == 1).all() and (_bits(got["ray"]) == _bits(rays)).all()
    assert (got["paths"] == exp["paths"]).all() and (got["casts"] == exp["casts"]).all(), name
    ex = exp["exact"]
    assert (_bits(got["samples"][ex]) == _bits(exp["samples"][ex])).all(), f"{name}: a miss or a roulette death is not the reference's bits"
    err = np.abs(got["samples"] - exp["samples"])
    assert (err <= T.REL_BAR * np.abs(exp["samples"])).all(), f"{name}: worst {float(err.max())}"
    assert (_bits(got["radiance"]) == _bits(T.reduce_samples(got["samples"]))).all()
    st = _stats(got["stats"])
    assert (st["rays"], st["casts"], st["samples"]) == (int(exp["paths"].sum()), int(exp["casts"].sum()), 64 * 3)
    assert gs.launch_status() == 0


def test_host_form_on_a_logical_device(gpu, ref_mesh, pt):
    from rt_amd import abi
    sc, gs, (o, q) = _scene(gpu, "rays", 4)
    ref = T.reference_samples(ref_mesh(4), sc, o[:70], q[:70], 3, T.SEED, 5, casts_oracle=pt)
    shim = abi.load_shim()
    assert shim.rt_hip_set_device_map((C.c_int * 3)(0, 0, 0), 3) == 0
    try:
        got = gpu.trace_rays_host(sc, ref["rays"], 3, T.SEED, index_first=5, device=2, want=ALL)
        with pytest.raises(gpu.ShimError):
            gpu.trace_rays_host(sc, ref["rays"][:4], 3, T.SEED, device=3)
    finally:
        assert shim.rt_hip_set_device_map(None, 0) == 0
    dev = _np(gs.trace_rays(ref["rays"], 3, T.SEED, index_first=5, want=ALL))
    for f in ALL:
        assert (np.asarray(got[f]) == dev[f]).all() if f in ("status", "paths", "casts") else (_bits(got[f]) == _bits(dev[f])).all(), f
    assert (got["paths"] == ref["paths"]).all() and got["stats"]["rays"] == int(ref["paths"].sum())
    assert gs.launch_status() == 0


def test_tie_to_the_renderer(gpu, pt):
    """a glass scene whose frame comes from a static member (a glass room beyond fp32's comfortable range: pt_render_tiles_big_refr
    whatever the sample count -- a small glass room takes the pooled refraction member, whose windowed sums add a path's terms one
    by one), at 1 spp: tracing every pixel's sample-0 camera ray GIVEN with index_first = 0 and S = 1 gives the frame bit for bit
    and its counters; on a plain room (pooled kernel) within assert_parity's bar"""
    import torch
    seed = 77
    for name, exact in (("glass", True), ("rays", False)):
        sc = util.class_scene(n_packed=4, refr=True, wide=True, depth=4) if exact else T.SCENES[name][1](4)
        sc.samples = 1
        gs = gpu.GpuScene(sc)
        img, _, st = gs.render_image(seed)
        kernel = gs.last_launch_kernel()
        print(f"{name}: frame from {kernel}, rays from {gs.trace_kernel_name()}")
        if exact:
            assert kernel == "pt_render_tiles_big_refr" and gs.trace_kernel_name() == "pt_trace_rays_big"
        else:
            assert kernel == "pt_render_tiles"
        w, h = sc.width, sc.height
        uv = np.zeros((w * h, 2))
        for p in range(w * h):
            r = pt.random_doubles(seed, p, 0, 2)
            uv[p] = ((p % w + r[0]) / (w - 1.0), (p // w + r[1]) / (h - 1.0))
        rays = gs.query_uv(uv, want=("ray",))["ray"]
        out = _np(gs.trace_rays(rays, 1, seed, want=("status", "radiance")))
        frame = img.cpu().numpy().reshape(-1, 3)
        ts = _stats(out["stats"])
        if exact:
            assert (out["radiance"].astype(np.float32).view(np.uint32) == frame.view(np.uint32)).all()
            assert (ts["rays"], ts["casts"], ts["tests"], ts["samples"]) == (st["rays"], st["casts"], st["tests"], w * h)
        else:
            util.assert_parity(frame, None, dict(rays=st["rays"], tests=st["tests"], casts=st["casts"]), out["radiance"], None,
                               dict(rays=ts["rays"], tests=ts["tests"], casts=ts["casts"]), name)
        assert gs.launch_status() == 0
        gs.close()
        sc.free()


def test_panorama(gpu):
    from rt_amd import scene as S
    sc, gs, _ = _scene(gpu, "rays", 4)
    objs, _ = util.scene_parts(sc)
    centre = tuple(float(x) for x in util.free_point(objs, np.zeros(3), clearance=0.5))   # the room's centre, outside every sphere
    pano, st = gs.render_panorama(16, 8, centre, 16, 5)
    direct = _np(gs.trace_rays(S.panorama_rays(16, 8, centre), 16, 5, want=("status", "radiance")))
    import torch
    torch.cuda.synchronize()
    p = pano.cpu().numpy()
    assert p.shape == (8, 16, 3) and (_bits(p.reshape(-1, 3)) == _bits(direct["radiance"])).all()
    assert (direct["status"] == 1).all() and p.max() > 10.0 / 255.0 * 1.5     # some pixel sees the light: above BACKGROUND


def test_zz_every_trace_form_was_compared(gpu):
    from rt_amd import abi
    shim = abi.load_shim()
    for k in range(shim.rt_hip_trace_kernel_count()):
        n = C.c_uint64(0)
        name = shim.rt_hip_trace_kernel_launches(k, C.byref(n)).decode()
        assert n.value > 0 and name in COMPARED, f"{name}: {n.value} launches, compared: {name in COMPARED}"
    print("worst |got - ref| / bar per scene:", {k: f"{v:.3e}" for k, v in WORST.items()})
    for sc, gs, _ in _CACHE.values():
        gs.close()
        sc.free()
    _CACHE.clear()

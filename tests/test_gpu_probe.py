"""Light probes on the GPU (include/rt_hip.h, "light probes"): the generator's rays equal the restatement (tests/probe_expected.py)
bit for bit; a bake is the stated composition of rt_hip_trace_rays calls and the stated fold, whatever the slices, in the device form
and the host form; a furnace whose answer the CPU derives; invalid probes; a glass scene through the pending-ray pool; the SH9
evaluation bit for bit; and one scene where the light has a direction."""
import ctypes as C

import numpy as np
import pytest

import probe_expected as P
import util

pytestmark = pytest.mark.gpu

DEPTH = 4
N, S = 16, 8          # the composition's probes and samples
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
    return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize])


def _host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _details(out):
    got = {k: _host(v) for k, v in out.items()}
    got["status"] = got["status"].view(np.uint32)
    return got


def _same(a, b):
    """bit-equal, a NaN matching any NaN"""
    return ((_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))).all()


def _cube_scene():
    """config 1's spheres and the cube of tests/golden/c3_cube.obj, as tests/test_gpu_parity.py sets it up"""
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
    sc = Sc.build_scene(1, 16, 16, 1, DEPTH)
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
        sc = {"room": lambda: Sc.build_scene(4, 16, 16, 1, DEPTH), "mesh": _cube_scene,
              "glass": lambda: util.class_scene(n_packed=4, refr=True, width=16, height=16, depth=DEPTH, samples=1),
              "furnace": P.furnace_scene}[name]()
        _CACHE[name] = (sc, gpu.GpuScene(sc))
    return _CACHE[name]


def _composition(gs, pos, nrm, samples, bias, radius):
    """what the bake is stated as: the restated rays, one rt_hip_trace_rays call with samples = 1 and index_first = 0, the restated
    fold of what it returns -> (rays, the call's outputs, sums)"""
    rays = P.probe_rays(pos, nrm, samples, P.SEED, bias=bias)
    out = gs.trace_rays(rays, 1, P.SEED, max_depth=DEPTH, origin_radius=radius, want=("status", "radiance", "samples", "ray"))
    got = {k: _host(v) for k, v in out.items()}
    got["status"] = got["status"].view(np.uint32)
    assert (_bits(got["ray"]) == _bits(rays)).all() and (_bits(got["samples"][:, 0]) == _bits(got["radiance"])).all()
    return rays, got, P.fold(rays, got["samples"][:, 0], samples, nrm, got["status"])


# ---- 1. the generator ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,s", P.SETS)
def test_rays_equal_the_restatement(gpu, n, s):
    cases = 0
    for dist in P.DISTANCES:
        pos, nrm = P.positions(n, dist), P.normals(n)
        for normals, bias in ((None, 0.0), (nrm, 0.0), (nrm, 2.0 ** -10)):
            want = P.probe_rays(pos, normals, s, P.SEED, bias=bias)
            got = _host(gpu.probe_rays(pos, s, P.SEED, normals=normals, bias=bias))
            assert got.shape == want.shape and (_bits(got) == _bits(want)).all(), (n, s, dist, bias, np.nonzero(_bits(got) != _bits(want))[0][:4])
            cases += 1
    pos, nrm = P.positions(n, 1.0), P.normals(n)
    for normals in (None, nrm):
        whole = P.probe_rays(pos, normals, s, P.SEED, bias=2.0 ** -10)
        for first, m in P.sub_ranges(n, s):
            got = _host(gpu.probe_rays(pos, s, P.SEED, normals=normals, bias=2.0 ** -10, k_first=first, n=m))
            assert got.shape == (m, 6) and (_bits(got) == _bits(whole[first:first + m])).all(), (n, s, first, m)
    print(f"N = {n}, S = {s}: {cases} cases and {2 * len(P.sub_ranges(n, s))} sub-ranges equal the restatement bit for bit")


def test_a_sub_range_writes_nothing_outside_itself(gpu):
    import torch
    from rt_amd import abi
    shim = abi.load_shim()
    pos = torch.as_tensor(P.positions(5, 1.0), device="cuda")
    buf = torch.full((80, 6), -7.0, dtype=torch.float64, device="cuda")
    p = abi.probe_params(abi.PROBE_SPHERE, 13, P.SEED)
    assert shim.rt_hip_probe_rays(C.c_void_p(pos.data_ptr()), None, 5, C.byref(p), 7, 50, C.c_void_p(buf[4:].data_ptr()), None) == 0
    got = _host(buf)
    want = P.probe_rays(P.positions(5, 1.0), None, 13, P.SEED, 7, 50)
    assert (got[:4] == -7.0).all() and (got[54:] == -7.0).all() and (_bits(got[4:54]) == _bits(want)).all()


# ---- 2. the furnace ----------------------------------------------------------------------------------------------------------------------
def test_furnace(gpu):
    """One sphere of radius 1000 and colour 0 that emits (1, 0.5, 0.25), probes within 10 of its centre, S = 64, depth 4.  The CPU
    knows every sample (probe_expected.furnace_radiance): the emission -- or, for a probe off the centre in the directions that point
    away from it, the background, because the reference's sphere test misses at tca < 0 even from inside; measured on the device:
    147 of 384 samples of six probes spread over the ball were the background, so "every sample is the emission" holds AT the centre
    only.  Sums and coefficients are the restated fold of those samples, bit for bit, for every probe.  For the three probes at the
    centre every sample is the emission exactly, coefficients 1 .. 8 estimate 0 and the hemisphere's E (bias 0: a biased origin is off
    the centre) estimates pi x emission, each within 6 standard errors, the error taken from the estimate's own 64 terms."""
    sc, gs = _scene(gpu, "furnace")
    f = P.FURNACE
    s, e, central = f["samples"], np.array(f["emission"]), f["central"]
    pos = P.furnace_positions()
    n = len(pos)
    assert (np.linalg.norm(pos, axis=1) <= 10.0).all() and (pos[:central] == 0).all()
    rays = P.probe_rays(pos, None, s, P.SEED)
    rad = P.furnace_radiance(rays)
    samples = _host(gs.trace_rays(rays, 1, P.SEED, max_depth=f["depth"], origin_radius=10.0, want=("samples",))["samples"])
    assert (samples[:, 0] == rad).all(), "a sample of the furnace is not what the CPU derives"
    assert (rad[:central * s] == e[None, :]).all(), "at the centre every sample is the emission"
    got = _details(gs.bake_probes(pos, s, P.SEED, max_depth=f["depth"], details=True))
    total = P.fold(rays, rad, s)
    coeff, coeff_f = P.resolve(total, s, P.SPHERE)
    assert (_bits(got["sum"]) == _bits(total)).all() and (_bits(got["coeff"]) == _bits(coeff)).all()
    assert (_bits(got["coeff_f"]) == _bits(coeff_f)).all() and (got["status"] == 1).all()
    assert got["stats"][3] == n * s
    terms = P.K[P.SPHERE] * P.sh_bases(rays[:, 3:]).reshape(n, s, 9)[:central, :, :, None] * e[None, None, None, :]
    se = terms.std(axis=1, ddof=1) / np.sqrt(s)
    ratio = np.abs(got["coeff"][:central, 1:]) / se[:, 1:]
    print(f"furnace: coefficients 1 .. 8 are at most {ratio.max():.2f} standard errors from 0")
    assert (ratio <= 6.0).all()
    # coefficient 0 is 4 pi Y0 x emission: 64 adds and three products, each within 2^-53 of exact
    assert (np.abs(got["coeff"][:central, 0] - terms[:, 0, 0]) <= 2.0 ** -46 * terms[:, 0, 0]).all()
    # the hemisphere
    nrm = P.normals(n)
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    hrays = P.probe_rays(pos, nrm, s, P.SEED)
    hrad = P.furnace_radiance(hrays)
    assert (hrad[:central * s] == e[None, :]).all()
    hgot = _details(gs.bake_irradiance(pos, nrm, s, P.SEED, max_depth=f["depth"], details=True))
    htotal = P.fold(hrays, hrad, s, nrm)
    hcoeff, hcoeff_f = P.resolve(htotal, s, P.HEMISPHERE)
    assert (_bits(hgot["sum"]) == _bits(htotal)).all() and (_bits(hgot["coeff"]) == _bits(hcoeff)).all()
    assert (_bits(hgot["coeff_f"]) == _bits(hcoeff_f)).all() and (hgot["status"] == 1).all()
    hterms = P.K[P.HEMISPHERE] * P.weights(hrays, s, nrm).reshape(n, s, 1)[:central, :, :, None] * e[None, None, None, :]
    hse = hterms.std(axis=1, ddof=1) / np.sqrt(s)
    hratio = np.abs(hgot["coeff"][:central] - np.pi * e[None, None, :]) / hse
    print(f"furnace: E is at most {hratio.max():.2f} standard errors from pi x emission")
    assert (hratio <= 6.0).all()
    E = _host(gs.bake_irradiance(pos, nrm, s, P.SEED, max_depth=f["depth"]))
    assert E.shape == (n, 3) and (_bits(E) == _bits(hcoeff.reshape(n, 3))).all()
    assert gs.launch_status() == 0


# ---- 3. the composition, 4. the slices ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["room", "mesh"])
@pytest.mark.parametrize("mode", ["sphere", "hemisphere"])
def test_bake_is_the_stated_composition_for_every_slice(gpu, name, mode):
    sc, gs = _scene(gpu, name)
    pos = P.positions(N, 3.0)
    nrm = P.normals(N) if mode == "hemisphere" else None
    bias = 2.0 ** -10 if mode == "hemisphere" else 0.0
    rays, call, total = _composition(gs, pos, nrm, S, bias, 4.0)
    assert (call["status"] == 1).all()
    coeff, coeff_f = P.resolve(total, S, P.HEMISPHERE if mode == "hemisphere" else P.SPHERE)

    def bake(slice_rays):
        if mode == "hemisphere":
            return _details(gs.bake_irradiance(pos, nrm, S, P.SEED, bias=bias, max_depth=DEPTH, origin_radius=4.0, slice_rays=slice_rays, details=True))
        return _details(gs.bake_probes(pos, S, P.SEED, max_depth=DEPTH, origin_radius=4.0, slice_rays=slice_rays, details=True))
    whole = bake(None)
    assert (_bits(whole["sum"]) == _bits(total)).all(), f"{name}: (c) the sums are not the stated fold of rt_hip_trace_rays' samples"
    assert (_bits(whole["coeff"]) == _bits(coeff)).all() and (_bits(whole["coeff_f"]) == _bits(coeff_f)).all()
    assert (whole["stats"] == call["stats"]).all(), (whole["stats"], call["stats"])
    assert (whole["status"] == 1).all()
    for slice_rays in (1, 7, S - 1, S, S + 1, N * S, 2 ** 31):                                        # (d)
        other = bake(slice_rays)
        for k in ("sum", "coeff", "coeff_f", "status", "stats"):
            assert (_bits(other[k]) == _bits(whole[k])).all(), (name, slice_rays, k)
    free = _details(gs.bake_probes(pos, S, P.SEED, max_depth=DEPTH, details=True)) if mode == "sphere" else None
    assert free is None or (_bits(free["coeff"]) == _bits(whole["coeff"])).all(), "origin_radius changes a bit"
    assert gs.launch_status() == 0


@pytest.mark.parametrize("mode", ["sphere", "hemisphere"])
def test_small_bake_for_slices_about_a_probe(gpu, mode):
    """3 probes x 5 samples: slices of 4 and 6 straddle a probe, 5 is a probe, 14, 15 and 16 are one short of the bake, the bake and
    more than it -- each gives the whole bake's sums, coefficients, status words and counters bit for bit, and that bake is the stated
    composition over rays 0 .. 14"""
    sc, gs = _scene(gpu, "room")
    n, s = 3, 5
    pos = P.positions(n, 3.0)
    nrm, bias = (P.normals(n), 2.0 ** -10) if mode == "hemisphere" else (None, 0.0)
    rays, call, total = _composition(gs, pos, nrm, s, bias, 4.0)
    assert (_bits(_host(gpu.probe_rays(pos, s, P.SEED, normals=nrm, bias=bias))) == _bits(rays)).all()

    def bake(slice_rays):
        if mode == "hemisphere":
            return _details(gs.bake_irradiance(pos, nrm, s, P.SEED, bias=bias, max_depth=DEPTH, origin_radius=4.0, slice_rays=slice_rays, details=True))
        return _details(gs.bake_probes(pos, s, P.SEED, max_depth=DEPTH, origin_radius=4.0, slice_rays=slice_rays, details=True))
    whole = bake(None)
    assert (_bits(whole["sum"]) == _bits(total)).all() and (whole["stats"] == call["stats"]).all()
    for slice_rays in (1, 4, 5, 6, 14, 15, 16):
        other = bake(slice_rays)
        for k in ("sum", "coeff", "coeff_f", "status", "stats"):
            assert (_bits(other[k]) == _bits(whole[k])).all(), (mode, slice_rays, k)
    assert gs.launch_status() == 0


# ---- 5. invalid probes ---------------------------------------------------------------------------------------------------------------------
def test_invalid_probes_are_nan_and_their_neighbours_untouched(gpu):
    """Probe k's rays have the indices [k S, (k + 1) S) whatever the other probes are: the neighbours of an invalid probe must hold
    the bits of a bake in which that probe's position (or normal) is an ordinary one."""
    sc, gs = _scene(gpu, "room")
    good = P.positions(7, 3.0)
    bad = good.copy()
    bad[1, 0], bad[3, 2], bad[5] = np.nan, np.inf, (-np.inf, 1.0, np.nan)
    invalid = np.array([False, True, False, True, False, True, False])
    for slice_rays in (None, 5):
        ref = _details(gs.bake_probes(good, S, P.SEED, max_depth=DEPTH, origin_radius=4.0, slice_rays=slice_rays, details=True))
        got = _details(gs.bake_probes(bad, S, P.SEED, max_depth=DEPTH, origin_radius=4.0, slice_rays=slice_rays, details=True))
        assert (got["status"] == np.where(invalid, 2, 1)).all() and (ref["status"] == 1).all()
        for k in ("sum", "coeff", "coeff_f"):
            assert np.isnan(got[k][invalid]).all() and (_bits(got[k][~invalid]) == _bits(ref[k][~invalid])).all(), (slice_rays, k)
    nrm = P.normals(7)
    bad_n = nrm.copy()
    bad_n[2, 1], bad_n[6, 0] = np.nan, np.inf
    invalid = np.array([False, False, True, False, False, False, True])
    ref = _details(gs.bake_irradiance(good, nrm, S, P.SEED, bias=0.5, max_depth=DEPTH, origin_radius=5.0, details=True))
    got = _details(gs.bake_irradiance(good, bad_n, S, P.SEED, bias=0.5, max_depth=DEPTH, origin_radius=5.0, details=True))
    assert (got["status"] == np.where(invalid, 2, 1)).all()
    assert np.isnan(got["coeff"][invalid]).all() and (_bits(got["coeff"][~invalid]) == _bits(ref["coeff"][~invalid])).all()
    assert gs.launch_status() == 0


# ---- 6. glass: the pending-ray pool -----------------------------------------------------------------------------------------------------------
def test_glass_scene_runs_through_the_pool(gpu):
    from rt_amd import abi
    sc, gs = _scene(gpu, "glass")
    pos = P.positions(8, 3.0)
    rays, call, total = _composition(gs, pos, None, 4, 0.0, 4.0)
    got = _details(gs.bake_probes(pos, 4, P.SEED, max_depth=DEPTH, origin_radius=4.0, slice_rays=5, details=True))
    assert gs.launch_status() == 0
    assert (_bits(got["sum"]) == _bits(total)).all() and np.isfinite(got["coeff"]).all() and (got["stats"] == call["stats"]).all()
    with pytest.raises(gpu.ShimError, match=r"\(-5\)"):          # RT_HIP_ELIMIT passes through from rt_hip_trace_rays
        gs.bake_probes(pos, 4, P.SEED, max_depth=33, origin_radius=4.0)
    with pytest.raises(gpu.ShimError, match=r"\(-2\)"):          # and its near_R rule
        gs.bake_probes(pos, 4, P.SEED, max_depth=DEPTH, origin_radius=1e15)
    assert gs.launch_status() == 0


# ---- 7. the evaluation ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 63, 64, 65])
def test_irradiance_equals_the_restatement(gpu, m):
    import torch
    rng = np.random.default_rng(m)
    n = 6
    coeff = rng.normal(0.0, 1.0, (n, 9, 3))
    coeff[1] = 0.0
    coeff[2, ::2] = -0.0
    coeff[3, :, 0], coeff[3, :, 1] = 5e-324, -2.2e-308
    coeff[4, 1:], coeff[4, 0] = 1e300, -1e300
    coeff[5, 4, 1], coeff[5, 0, 2] = np.nan, np.inf
    index = rng.integers(0, n, m)
    index[m // 2] = n + (7 if m > 1 else 0)          # out of range (m == 1: the only entry)
    if m > 2:
        index[0] = 2 ** 32 - 1
    normals = rng.normal(0.0, 1.0, (m, 3))
    normals[::3] /= np.linalg.norm(normals[::3], axis=1)[:, None]
    want = P.irradiance(coeff, index, normals)
    got = _host(gpu.probe_irradiance(torch.as_tensor(coeff, device="cuda"), index, normals))
    assert got.shape == (m, 3) and _same(got, want), np.nonzero(~((_bits(got) == _bits(want)) | (np.isnan(got) & np.isnan(want))))
    assert np.isnan(got[index >= n]).all() and (np.isnan(got) == np.isnan(want)).all()


def test_resolve_alone(gpu):
    import torch
    rng = np.random.default_rng(3)
    for bases, mode in ((9, P.SPHERE), (1, P.HEMISPHERE)):
        total = rng.normal(0.0, 100.0, (5, bases, 3))
        total[0, 0] = (np.nan, -0.0, 1e308)
        for samples in (1, 3, 64):
            coeff, coeff_f = gpu.probe_resolve(torch.as_tensor(total, device="cuda"), samples)
            want, want_f = P.resolve(total, samples, mode)
            assert _same(_host(coeff), want) and _same(_host(coeff_f), want_f), (bases, samples)


# ---- 8. the light has a direction ----------------------------------------------------------------------------------------------------------------
def test_a_light_above_the_probe(gpu):
    """a black room and one bright emitter of radius 2 at (0, 0, 5): of 256 directions about 4 % reach it.  The z coefficient is
    positive in every channel and a surface facing the light receives more than one facing away."""
    from rt_amd import abi, scene as Sc
    objs = [dict(flags=abi.M_DEFAULT, radius=1000.0, center=(0.0, 0.0, 0.0), color=(0.0, 0.0, 0.0), emission=(0.0, 0.0, 0.0)),
            dict(flags=abi.M_DEFAULT, radius=2.0, center=(0.0, 0.0, 5.0), color=(0.0, 0.0, 0.0), emission=(40.0, 30.0, 20.0))]
    sc = Sc.custom_scene(objs, 16, 16, 1, DEPTH, (0.0, 0.0, -10.0), (0.0, 0.0, 0.0))
    gs = gpu.GpuScene(sc)
    sh = gs.bake_probes([[0.0, 0.0, 0.0]], 256, P.SEED, max_depth=DEPTH)
    E = _host(gpu.probe_irradiance(sh, [0, 0], [[0.0, 0.0, 1.0], [0.0, 0.0, -1.0]]))
    coeff = _host(sh)
    assert gs.launch_status() == 0
    print("coeff[0][2] =", coeff[0, 2], " E(+z) =", E[0], " E(-z) =", E[1])
    assert (coeff[0, 2] > 0).all() and (coeff[0, 0] > 0).all()
    assert (E[0] > E[1]).all()
    up = _host(gs.bake_irradiance([[0.0, 0.0, 0.0]] * 2, [[0.0, 0.0, 1.0], [0.0, 0.0, -1.0]], 256, P.SEED, max_depth=DEPTH))
    assert (up[0] > 0).all() and (up[1] == 0).all(), "the hemisphere facing away sees the black room only"
    gs.close()
    sc.free()


# ---- 9. the host form, on a logical device ---------------------------------------------------------------------------------------------------------
def test_host_form_on_a_logical_device(gpu):
    from rt_amd import abi
    shim = abi.load_shim()
    sc, gs = _scene(gpu, "room")
    pos, nrm = P.positions(N, 3.0), P.normals(N)
    dev = _details(gs.bake_probes(pos, S, P.SEED, max_depth=DEPTH, details=True))
    on0 = gpu.bake_probes_host(sc, pos, S, P.SEED, max_depth=DEPTH)
    assert shim.rt_hip_set_device_map((C.c_int * 2)(0, 0), 2) == 0
    try:
        on1 = gpu.bake_probes_host(sc, pos, S, P.SEED, max_depth=DEPTH, device=1)
        h1 = gpu.bake_probes_host(sc, pos, S, P.SEED, normals=nrm, bias=0.25, max_depth=DEPTH, device=1)
        with pytest.raises(gpu.ShimError):
            gpu.bake_probes_host(sc, pos, S, P.SEED, max_depth=DEPTH, device=2)
    finally:
        assert shim.rt_hip_set_device_map(None, 0) == 0
    for a, b in zip(on0[:3], on1[:3]):
        assert (_bits(a) == _bits(b)).all()
    assert on0[3] == on1[3] == dict(zip(("rays", "casts", "tests", "samples"), (int(v) for v in dev["stats"])))
    assert (_bits(on0[0]) == _bits(dev["coeff"])).all() and (_bits(on0[1]) == _bits(dev["coeff_f"])).all() and (on0[2] == dev["status"]).all()
    hdev = _details(gs.bake_irradiance(pos, nrm, S, P.SEED, bias=0.25, max_depth=DEPTH, details=True))
    assert (_bits(h1[0]) == _bits(hdev["coeff"])).all() and (h1[2] == 1).all()


def test_cli_prints_a_probe(gpu):
    """raytracer -k x,y,z: the 27 coefficients of one probe in the chosen config, %.17g, equal to the host form's"""
    import os
    import re
    import subprocess
    from rt_amd import abi, scene as Sc
    cli = os.path.join(os.path.dirname(abi.HOST_PATH), "raytracer")
    at = (0.5, 1.0, 2.0)
    r = subprocess.run([cli, "-c", "1", "-s", "16", "-d", str(DEPTH), "-r", str(P.SEED), "-k", ",".join(f"{v:g}" for v in at)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    rows = re.findall(r"^sh\[(\d)\] = (\S+) (\S+) (\S+)$", r.stdout, re.M)
    assert [int(j) for j, *_ in rows] == list(range(9)) and "status = 1" in r.stdout
    got = np.array([[float(v) for v in row[1:]] for row in rows])
    sc = Sc.build_scene(1, 320, 180, 16, DEPTH)
    want, _, status, _ = gpu.bake_probes_host(sc, [at], 16, P.SEED, max_depth=DEPTH)
    sc.free()
    assert status[0] == 1 and (_bits(got) == _bits(want[0])).all()
    for bad in ("1,2", "1,2,x", "1,2,3,4", "nan,0,0"):
        r = subprocess.run([cli, "-c", "1", "-s", "4", "-k", bad], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "Usage" in r.stderr, bad


def test_zz_close(gpu):
    for sc, gs in _CACHE.values():
        gs.close()
        sc.free()
    _CACHE.clear()

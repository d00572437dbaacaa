"""A deforming mesh: GpuScene.update_vertices (rt_hip_scene_update_vertices, raytracer.c_amd/csrc/scene_update.hip).

A hierarchy only decides which triangles get the exact test, so after an update everything equals a freshly created scene's:
  1. the records (read_triangles: bytes, NaN equal to NaN), the mesh bound, reach, hull_facets, kernel_name and mesh_round, over
     the meshes at which a path can go wrong, both builders, deformations (a) identity, (b) scale and wobble, (c) mirror,
     (d) squash and restore, (e) translate by 40; the frame of every step equals the fresh scene's bits;
  2. the tree equals BvhRefit (tests/bvh_refit_harness.cpp) byte for byte, refs and order as before the update, and under (a) a
     device-built tree's nodes do not change at all;
  3. frames of every hierarchy-walking render form (and the flat-filter _tri form) meet the oracle on the deformed scene through
     util.assert_parity and equal the fresh scene's image, bytes and counters;
  4. ray queries, radiance queries, pixel queries and first-hit buffers after (b) on the 10,240-triangle sphere equal the fresh
     scene's bits, the ray query also the compiled reference;
  5. ten updates in a row: every frame meets the oracle, update_info counts 10, the pools do not grow;
  6. refusals leave records and frame as they were;
  7. the PT_DIAG re-check of the skipping rules on an updated scene (tests/scene_update_diag_child.py): 0 violations;
  8. the C host: with rt_set_scene_updates(1) a moved mesh updates the cached context, also on 2 logical devices; with the
     default 0 it rebuilds.
"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bvh_sweep_meshes as M
import scene_update_meshes as U
from conftest import SEED
from util import assert_parity, class_scene, fixed_point_floor

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAME = dict(width=64, height=40, samples=2, depth=16)
MESHES = ["n15", "n16", "n17", "n241", "n257", "duplicated", "signed_zeros", "uv_sphere"]
BUILDERS = ["host", "device"]


@pytest.fixture(scope="module")
def gpu():
    import torch
    from rt_amd import abi, gpu as G
    assert abi.load_shim().rt_hip_device_count() >= 1, "no HIP device: the GPU tests must run on the GPU box"
    assert torch.cuda.is_available()
    yield G
    abi.load_host().rt_set_scene_updates(0)
    abi.load_shim().rt_hip_set_bvh_builder(0)
    abi.load_shim().rt_hip_set_device_map(None, 0)


@pytest.fixture(scope="module")
def refit(tmp_path_factory):
    return U.Refit(U.compile_harness(tmp_path_factory.mktemp("refit")))


def mesh_scene(tris, width=64, height=40, samples=2, depth=16):
    """as tests/test_gpu_bvh_device.py: a floor-less scene of one light sphere and the mesh"""
    from rt_amd import abi, scene as S
    objs = [dict(flags=abi.M_DEFAULT, radius=4.0, center=(0, 18, 0), color=(1, 1, 1), emission=(8, 8, 8))]
    return S.custom_scene(objs, width, height, samples, depth, (0, 0, 4), (0, 0, 0),
                          meshes=[dict(flags=abi.M_DEFAULT, color=(0.8, 0.7, 0.6), triangles=np.asarray(tris, dtype=np.float64))])


def vertex_view(sc, m=0):
    """the (3 n, 5) float64 view of mesh m's vertex array (pos xyz, tex uv): writing it moves the host scene"""
    n = 3 * sc.meshes[m].mesh.num_triangles
    return np.ctypeslib.as_array(C.cast(sc.meshes[m].mesh.vertices, C.POINTER(C.c_double)), shape=(n, 5))


def tris_of(sc):
    return np.concatenate([vertex_view(sc, m)[:, :3].reshape(-1, 3, 3) for m in range(sc.n_meshes)]).copy()


def move_scene(sc, tris):
    """writes the corners (n, 3, 3) into the host scene's vertex arrays, mesh by mesh"""
    at = 0
    for m in range(sc.n_meshes):
        v = vertex_view(sc, m)
        v[:, :3] = tris[at:at + len(v) // 3].reshape(-1, 3)
        at += len(v) // 3


def state(gs):
    s = gs.read_triangles()
    s.update(bounds=gs.bounds(), hull=gs.hull_facets(), kernel=gs.kernel_name(), whitted=gs.kernel_name("whitted"))
    return s


def same_bits_or_nan(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != np.float64:
        return np.array_equal(a, b)
    return bool(((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))).all())


def assert_same_state(got, want, what):
    for f in ("geom", "normal", "entry", "object"):
        assert same_bits_or_nan(got[f], want[f]), f"{what}: {f} differs from the fresh scene's"
    gb, wb = got["bounds"], want["bounds"]
    assert gb["mesh_center"] == wb["mesh_center"], f"{what}: mesh centre {gb['mesh_center']} != {wb['mesh_center']}"   # by value
    for f in ("mesh_radius", "reach", "mesh_round"):
        assert gb[f] == wb[f], f"{what}: {f} {gb[f]} != {wb[f]}"
    assert np.float64(gb["mesh_radius"]).view(np.uint64) == np.float64(wb["mesh_radius"]).view(np.uint64)
    for f in ("hull", "kernel", "whitted"):
        assert got[f] == want[f], f"{what}: {f} {got[f]} != {want[f]}"


def frame(gs, integrator="path"):
    img, img8, st = gs.render_image(SEED, integrator=integrator)
    assert gs.launch_status() == 0
    return img.cpu().numpy(), img8.cpu().numpy(), st, gs.last_launch_kernel()


def assert_same_frame(a, b, what):
    assert a[3] == b[3], f"{what}: launched {a[3]}, the fresh scene {b[3]}"
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)), f"{what}: float frame differs from the fresh scene's"
    assert np.array_equal(a[1], b[1]) and a[2] == b[2], f"{what}: bytes or counters differ from the fresh scene's"


def as_input(gpu, tris, k):
    """the new positions as a device tensor (even k: the device entry, no host copy) or a numpy array (odd k: the host entry)"""
    import torch
    return torch.tensor(tris, dtype=torch.float64, device="cuda") if k % 2 == 0 else np.ascontiguousarray(tris)


@pytest.mark.parametrize("builder", BUILDERS)
@pytest.mark.parametrize("name", MESHES)
def test_update_equals_a_fresh_scene(gpu, refit, name, builder):
    tris = np.array(M.mesh(name)) * (1.0 if name == "uv_sphere" else 3.0)
    gs = gpu.GpuScene(mesh_scene(tris), bvh=builder)
    nodes0, order0 = gs.bvh_read()
    before = frame(gs)
    steps = [("identity", U.identity(tris)), ("scale_wobble", U.scale_wobble(tris)), ("mirror", U.mirror(tris)),
             ("squash", U.squash(tris)), ("restore", U.identity(tris)), ("translate", U.translate(tris))]
    rounds, kernels, nodes_prev = [], [], nodes0
    for k, (step, new) in enumerate(steps):
        what = f"{name} {builder} {step}"
        gs.update_vertices(as_input(gpu, new, k))
        fresh = gpu.GpuScene(mesh_scene(new), bvh=builder)
        assert_same_state(state(gs), state(fresh), what)
        # the tree: BvhRefit of the tree before this update, byte for byte; refs and order never move
        nodes, order = gs.bvh_read()
        want = refit.refit(nodes_prev, order0, M.geom(new))
        assert np.array_equal(order, order0), f"{what}: the leaf order changed"
        assert np.array_equal(nodes[:, 12:].view(np.uint64), nodes0[:, 12:].view(np.uint64)), f"{what}: refs or padding changed"
        bad = np.nonzero((nodes.view(np.uint64) != want.view(np.uint64)).any(axis=1))[0]
        assert bad.size == 0, f"{what}: {bad.size} of {len(nodes)} nodes differ from BvhRefit's, first {bad[:4]}"
        U.check_refitted(nodes0, order0, nodes, M.geom(new), what)
        if builder == "device" and step in ("identity", "restore"):
            assert np.array_equal(nodes.view(np.uint64), nodes0.view(np.uint64)), f"{what}: a device tree's nodes must return"
        nodes_prev = nodes
        got, exp = frame(gs), frame(fresh)
        assert_same_frame(got, exp, what)
        if step in ("identity", "restore"):
            assert_same_frame(got, before, what + " against the frame before any update")
        rounds.append(gs.bounds()["mesh_round"])
        kernels.append(got[3])
        fresh.close()
    assert gs.update_info()["updates"] == len(steps) and gs.update_info()["last_seconds"] > 0
    info = gs.bvh_info()
    assert info["builder"] == builder and info["n_nodes"] == len(nodes0)
    if name == "uv_sphere":   # (d): the squashed sphere is a disc, its bounding sphere no target: the member changes and changes back
        assert rounds[2:5] == [True, False, True], rounds
        assert "_sph" in before[3] and "_sph" in kernels[2] and "_sph" not in kernels[3] and kernels[4] == before[3], kernels
    gs.close()


RENDER_FORMS = [
    (dict(n_packed=4, tris=400), "path", "pt_render_tiles_tri_queued"),
    (dict(n_packed=4, tris=400, chk=True), "path", "pt_render_tiles_tri_queued_chk"),
    (dict(n_packed=4, tris=400, round_mesh=True), "path", "pt_render_tiles_tri_queued_sph"),
    (dict(n_packed=4, tris=400, mesh_refr=True), "path", "pt_render_tiles_tri_queued_refr"),
    (dict(n_packed=4, tris=400, round_mesh=True, mesh_refr=True), "path", "pt_render_tiles_tri_queued_refr_sph"),
    (dict(n_packed=4, tris=400, wide=True), "path", "pt_render_tiles_tri_big"),
    (dict(n_packed=4, tris=400), "whitted", "pt_whitted_tiles_tri_big"),
    (dict(n_packed=300, tris=60), "whitted", "pt_whitted_tiles_mem"),
    (dict(n_packed=4, tris=60), "path", "pt_render_tiles_tri"),          # <= 256 primitives: the flat filter, rebuilt from entry_src
]


@pytest.mark.parametrize("cls,integrator,kernel", RENDER_FORMS, ids=[r[2] for r in RENDER_FORMS])
def test_frames_after_an_update(gpu, pt, cls, integrator, kernel):
    base = class_scene(**dict(cls, **FRAME))
    tris = tris_of(base)
    scenes = {b: gpu.GpuScene(base, bvh=b) for b in BUILDERS}
    for k, deform in enumerate(("scale_wobble", "mirror")):
        new = U.DEFORMATIONS[deform](tris)
        moved = class_scene(**dict(cls, **FRAME))
        move_scene(moved, new)
        mean, rgb8, ost = pt.render_pixels(moved, SEED, integrator=integrator)
        fresh = gpu.GpuScene(moved, bvh="host")
        exp = frame(fresh, integrator)
        assert exp[3] == kernel, f"the fresh {deform} scene took {exp[3]}"
        fresh.close()
        for b, gs in scenes.items():
            what = f"{kernel} {deform} {b} tree"
            gs.update_vertices(as_input(gpu, new, k + (b == "host")))
            got = frame(gs, integrator)
            assert_parity(got[0], got[1], got[2], mean, rgb8, ost, what=what, hdr=True, abs_floor=fixed_point_floor(moved))
            assert_same_frame(got, exp, what)
        moved.free()
    for gs in scenes.values():
        gs.close()
    base.free()


def _np(out):
    import torch
    torch.cuda.synchronize()
    res = {f: t.cpu().numpy() for f, t in out.items()}
    return {f: np.ascontiguousarray(x).view(np.uint8) for f, x in res.items()}


def test_queries_and_first_hit_buffers_after_an_update(gpu, ref_mesh):
    """after (b) on the 10,240-triangle sphere: the four query forms equal the fresh scene's bits; the ray query equals the
    compiled reference, as test_ray_queries_through_a_device_tree compares it"""
    import query_expected as Q
    import refine_expected as R
    tris = np.array(M.mesh("uv_sphere"))
    new = U.scale_wobble(tris)
    moved = mesh_scene(new)
    rays = Q.ray_set(moved)
    exp = Q.expected(ref_mesh(16), moved, rays=rays)
    pixels = R.pixel_list(moved.width, moved.height)
    for b in BUILDERS:
        gs, fresh = gpu.GpuScene(mesh_scene(tris), bvh=b), gpu.GpuScene(moved, bvh=b)
        gs.update_vertices(as_input(gpu, new, 0))
        got = {f: t.cpu().numpy() for f, t in gs.query_rays(rays).items()}
        msg = Q.mismatch(got, exp)
        assert not msg, f"{b} tree: {msg}"
        assert (got["prim"].view(np.uint32) != 0xFFFFFFFF).sum() > 20, "the rays must meet triangles"
        calls = {"query_rays": lambda s: _np(s.query_rays(rays)),
                 "trace_rays": lambda s: _np(s.trace_rays(rays[:65], 2, SEED, want=("status", "radiance", "samples", "paths", "casts"))),
                 "trace_pixels": lambda s: _np(s.trace_pixels(pixels, 2, SEED, want=("status", "radiance", "samples", "paths", "casts"))),
                 "render_aov": lambda s: {f: np.ascontiguousarray(x).view(np.uint8) for f, x in s.aov_image(SEED, 2).items()}}
        for form, call in calls.items():
            a, e = call(gs), call(fresh)
            assert a.keys() == e.keys()
            for f in a:
                assert np.array_equal(a[f], e[f]), f"{form} {b} tree: {f} differs from the fresh scene's"
            assert gs.launch_status() == 0
        gs.close()
        fresh.close()


def test_ten_updates_in_a_row(gpu, pt):
    from rt_amd import abi
    shim = abi.load_shim()
    tris = np.array(M.mesh("n257")) * 3.0
    gs = gpu.GpuScene(mesh_scene(tris), bvh="device")
    frame(gs)

    def pools():
        park, pend = C.c_size_t(0), C.c_size_t(0)
        assert shim.rt_hip_pool_bytes(0, C.byref(park), C.byref(pend)) == 0
        return park.value, pend.value

    gs.update_vertices(tris)          # the first update makes the level array
    frame(gs)
    pools0, k0 = pools(), gs.update_info()["updates"]
    for k in range(10):
        new = U.scale_wobble(tris, phase=0.3 * (k + 1))
        gs.update_vertices(as_input(gpu, new, k))
        moved = mesh_scene(new)
        mean, rgb8, ost = pt.render_pixels(moved, SEED)
        got = frame(gs)
        assert_parity(got[0], got[1], got[2], mean, rgb8, ost, what=f"wobble frame {k}", hdr=True, abs_floor=fixed_point_floor(moved))
    assert gs.update_info()["updates"] == k0 + 10
    assert pools() == pools0, "an update must not grow the device's pools"
    gs.close()


def test_refusals_leave_the_scene_alone(gpu):
    import torch
    from rt_amd import abi
    tris = np.array(M.mesh("n257")) * 3.0
    gs = gpu.GpuScene(mesh_scene(tris), bvh="device")
    s0, f0 = state(gs), frame(gs)
    moved = U.scale_wobble(tris)

    def refused(call, word):
        with pytest.raises(gpu.ShimError) as e:
            call()
        assert f"({abi.EINVAL})" in str(e.value) and word in str(e.value), str(e.value)
        assert_same_state(state(gs), s0, word)
        assert_same_frame(frame(gs), f0, word)
        assert gs.update_info()["updates"] == 0

    shim = abi.load_shim()
    refused(lambda: gpu._check(shim.rt_hip_scene_update_vertices_host(gs.handle, moved.ctypes.data, len(tris) - 1), "update"), "count")
    refused(lambda: gpu._check(shim.rt_hip_scene_update_vertices_host(gs.handle, None, len(tris)), "update"), "required")
    acc = gs.accumulate(SEED, 4)
    refused(lambda: gs.update_vertices(moved), "accumulation")
    acc.close()
    bad = moved.copy()
    bad[100, 1, 2] = np.nan
    refused(lambda: gs.update_vertices(bad), "non-finite")
    refused(lambda: gs.update_vertices(torch.tensor(bad, device="cuda")), "non-finite")
    bad = moved.copy()
    bad[7, 0, 0] = 1e301
    refused(lambda: gs.update_vertices(bad), "non-finite")
    refused(lambda: gs.update_vertices(torch.tensor(moved)), "device memory")        # a host tensor at the device entry
    balls = gpu.GpuScene(class_scene(n_packed=4, **FRAME))
    with pytest.raises(gpu.ShimError) as e:
        gpu._check(shim.rt_hip_scene_update_vertices_host(balls.handle, moved.ctypes.data, 0), "update")
    assert "no triangles" in str(e.value)
    balls.close()
    # and once nothing stands in the way, the same positions go through
    gs.update_vertices(moved)
    fresh = gpu.GpuScene(mesh_scene(moved), bvh="device")
    assert_same_state(state(gs), state(fresh), "after the refusals")
    assert_same_frame(frame(gs), frame(fresh), "after the refusals")
    assert gs.update_info()["updates"] == 1
    fresh.close()
    gs.close()


def test_skipping_rules_hold_on_an_updated_scene():
    """one frame of the 10,240-triangle sphere, scaled and wobbled in place, through the PT_DIAG build: the exhaustive re-checks
    of the conservative rules (filter, pre-tests, probe, hull facets) find nothing"""
    env = dict(os.environ, RT_HIP_SHIM_PATH=os.path.join(ROOT, "raytracer.c_amd", "csrc", "librt_hip_diag.so"))
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "scene_update_diag_child.py")], env=env, capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    rec = json.loads(out.stdout.strip().splitlines()[-1])
    print(rec)
    assert rec["updates"] == 1 and rec["violations"] == 0
    assert rec["leaf_pretests"] > 0 and rec["casts"] > 0, "the check was not vacuous"


def test_c_host_updates_the_cached_scene(gpu):
    """rt_hip_render_image under rt_set_scene_updates: a moved mesh updates the cached context in place (one build, one update),
    the frame is a fresh process-level render's, also on 2 logical devices; with the default 0 the second call rebuilds"""
    from rt_amd import abi
    shim, host = abi.load_shim(), abi.load_host()
    cls = dict(dict(n_packed=4, tris=400, round_mesh=True), **FRAME)
    base = class_scene(**cls)
    moved = class_scene(**cls)
    move_scene(moved, U.scale_wobble(tris_of(base)))
    for map_, n_dev in ((None, 1), ((C.c_int * 2)(0, 0), 2)):
        assert shim.rt_hip_set_device_map(map_, 2 if map_ is not None else 0) == 0
        host.rt_set_scene_updates(0)
        shim.rt_hip_release_cache()
        want = gpu.render_image_host(moved, SEED, n_devices=n_dev)          # a fresh context for the moved scene
        shim.rt_hip_release_cache()
        for on in (1, 0):
            host.rt_set_scene_updates(on)
            shim.rt_hip_release_cache()
            b0, u0 = shim.rt_hip_cache_builds(), shim.rt_hip_cache_updates()
            gpu.render_image_host(base, SEED, n_devices=n_dev)
            got = gpu.render_image_host(moved, SEED, n_devices=n_dev)
            again = gpu.render_image_host(moved, SEED, n_devices=n_dev)
            builds, updates = shim.rt_hip_cache_builds() - b0, shim.rt_hip_cache_updates() - u0
            assert (builds, updates) == ((1, 1) if on else (2, 0)), f"updates {on}, {n_dev} devices: {builds} builds, {updates} updates"
            for other in (got, again):
                assert np.array_equal(want[0].view(np.uint32), other[0].view(np.uint32)) and np.array_equal(want[1], other[1])
                assert want[2] == other[2]
    host.rt_set_scene_updates(0)
    shim.rt_hip_set_device_map(None, 0)
    shim.rt_hip_release_cache()
    base.free()
    moved.free()

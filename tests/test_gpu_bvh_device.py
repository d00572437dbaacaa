"""The triangle hierarchy built on the device (raytracer.c_amd/csrc/bvh_device.hip, GpuScene(bvh="device")).

  1. tree: over the mesh set of tests/bvh_sweep_meshes.py, the nodes and the order read back from a device-built scene equal
     BvhSweep's (raytracer.c_amd/csrc/bvh_build.h, through tests/bvh_sweep_harness.cpp) byte for byte, and so do the depth,
     the node count and the cost rt_hip_scene_bvh_info reports;
  2. two builds of one mesh are byte-equal;
  3. frames: one scene per hierarchy-walking form at 64 x 40, 2 spp, depth 16: the frame of the device-built scene meets the
     oracle through util.assert_parity and equals the host-built scene's bytes and counters, the launch's kernel asserted
     (the _chk, _sph, _refr and _refr_sph variants of the queued form included); pt_query_rays_tri_big, pt_trace_rays_tri_big,
     pt_trace_pixels_tri_big and pt_aov_tiles_tri_big meet the compiled reference as tests/test_gpu_query.py, test_gpu_trace.py,
     test_gpu_refine.py and test_gpu_aov.py compare them, through either tree, with the same bits, the launched form counted;
  4. every triangle twice: the first-index tie holds through a device tree;
  5. the skipping rules re-checked by the PT_DIAG build on a device tree (tests/bvh_device_diag_child.py): 0 violations;
  6. the C host: rt_hip_render_image after rt_hip_set_bvh_builder(1) gives the frame before and rebuilds once, also on logical
     device 2 of a (0, 0, 0) map; the CLI's -b 1 writes the same PNG bytes.
"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bvh_sweep_meshes as M
from conftest import SEED
from util import assert_parity, class_scene, fixed_point_floor

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAME = dict(width=64, height=40, samples=2, depth=16)


@pytest.fixture(scope="module")
def gpu():
    import torch
    from rt_amd import abi, gpu as G
    assert abi.load_shim().rt_hip_device_count() >= 1, "no HIP device: the GPU tests must run on the GPU box"
    assert torch.cuda.is_available()
    yield G
    abi.load_shim().rt_hip_set_bvh_builder(0)
    abi.load_shim().rt_hip_set_device_map(None, 0)


@pytest.fixture(scope="module")
def sweep(tmp_path_factory):
    return M.Sweep(M.compile_harness(tmp_path_factory.mktemp("sweep")))


def mesh_scene(tris, width=64, height=40, samples=2, depth=16):
    """a floor-less scene of one light sphere and the mesh (scene.custom_scene fills the vertex array from the numpy array at once)"""
    from rt_amd import abi, scene as S
    objs = [dict(flags=abi.M_DEFAULT, radius=4.0, center=(0, 18, 0), color=(1, 1, 1), emission=(8, 8, 8))]
    return S.custom_scene(objs, width, height, samples, depth, (0, 0, 4), (0, 0, 0),
                          meshes=[dict(flags=abi.M_DEFAULT, color=(0.8, 0.7, 0.6), triangles=np.asarray(tris, dtype=np.float64))])


@pytest.mark.parametrize("name", list(M.MESHES))
def test_tree_equals_the_restatement(gpu, sweep, name):
    tris = M.mesh(name)
    want = sweep.build(M.geom(tris))
    assert want["rc"] == 0
    sc = mesh_scene(tris)
    gs = gpu.GpuScene(sc, bvh="device")
    info = gs.bvh_info()
    nodes, order = gs.bvh_read()
    again = gpu.GpuScene(sc, bvh="device")
    nodes2, order2 = again.bvh_read()
    again.close()
    gs.close()
    print(f"{name}: {len(tris)} triangles, {info['n_nodes']} nodes, depth {info['depth']} of {info['max_depth']}, "
          f"cost {info['tree_cost']:.3f}, device build {1e3 * info['build_seconds']:.3f} ms")
    assert (info["builder"], info["depth"], info["max_depth"], info["n_nodes"]) == \
        ("device", want["depth"], want["max_depth"], want["n_nodes"])
    assert np.array_equal(order, want["order"]), f"{name}: order differs first at {np.nonzero(order != want['order'])[0][:4]}"
    got, exp = nodes.view(np.uint64), want["nodes"].view(np.uint64)
    bad = np.nonzero((got != exp).any(axis=1))[0]
    assert bad.size == 0, f"{name}: {bad.size} of {len(got)} nodes differ, first {bad[:4]}: {nodes[bad[0]]} != {want['nodes'][bad[0]]}"
    assert info["tree_cost"] == want["cost"]
    assert np.array_equal(order2, order) and np.array_equal(nodes2.view(np.uint64), got), "two builds of one mesh differ"


def test_default_is_the_host_builder(gpu):
    sc = class_scene(n_packed=4, tris=400, **FRAME)
    gs = gpu.GpuScene(sc)
    info = gs.bvh_info()
    nodes, order = gs.bvh_read()
    gs.close()
    assert info["builder"] == "host" and info["n_nodes"] == len(nodes) > 1 and sorted(order.tolist()) == list(range(400))
    with pytest.raises(ValueError):
        gpu.GpuScene(sc, bvh="gpu")


def _pair(gpu, sc):
    return gpu.GpuScene(sc, bvh="host"), gpu.GpuScene(sc, bvh="device")


RENDER_FORMS = [
    (dict(n_packed=4, tris=400), "path", 0, "pt_render_tiles_tri_queued"),
    (dict(n_packed=4, tris=400, chk=True), "path", 0, "pt_render_tiles_tri_queued_chk"),
    (dict(n_packed=4, tris=400, round_mesh=True), "path", 0, "pt_render_tiles_tri_queued_sph"),
    (dict(n_packed=4, tris=400, mesh_refr=True), "path", 0, "pt_render_tiles_tri_queued_refr"),
    (dict(n_packed=4, tris=400, round_mesh=True, mesh_refr=True), "path", 0, "pt_render_tiles_tri_queued_refr_sph"),
    (dict(n_packed=4, tris=400, wide=True), "path", 0, "pt_render_tiles_tri_big"),
    (dict(n_packed=4, tris=400), "whitted", 0, "pt_whitted_tiles_tri_big"),
    (dict(n_packed=300, tris=60), "whitted", 0, "pt_whitted_tiles_mem"),
]


@pytest.mark.parametrize("cls,integrator,faults,kernel", RENDER_FORMS, ids=[r[3] for r in RENDER_FORMS])
def test_frames_through_a_device_tree(gpu, pt, cls, integrator, faults, kernel):
    sc = class_scene(**dict(cls, **FRAME))
    mean, rgb8, ost = pt.render_pixels(sc, SEED, integrator=integrator)
    frames = []
    for gs in _pair(gpu, sc):
        img, img8, st = gs.render_image(SEED, integrator=integrator)
        assert gs.last_launch_kernel() == kernel, f"{gs.bvh_info()['builder']}: took {gs.last_launch_kernel()}"
        assert gs.launch_status() == 0
        frames.append((img.cpu().numpy(), img8.cpu().numpy(), st))
        gs.close()
    assert_parity(frames[1][0], frames[1][1], frames[1][2], mean, rgb8, ost, what=f"{kernel} device tree", hdr=True,
                  abs_floor=fixed_point_floor(sc))
    assert np.array_equal(frames[0][0].view(np.uint32), frames[1][0].view(np.uint32)), "float frame differs from the host tree's"
    assert np.array_equal(frames[0][1], frames[1][1]) and frames[0][2] == frames[1][2]
    sc.free()


def _np(out):
    import torch
    torch.cuda.synchronize()
    res = {f: t.cpu().numpy() for f, t in out.items()}
    res = {f: (x.view(np.uint32) if x.dtype == np.int32 else x) for f, x in res.items()}
    for f in ("paths", "casts"):
        if f in res:
            res[f] = res[f].view(np.uint64)
    return res


def _same_bits(a, b, what):
    assert a.keys() == b.keys()
    for f in a:
        assert np.array_equal(np.ascontiguousarray(a[f]).view(np.uint8), np.ascontiguousarray(b[f]).view(np.uint8)), f"{what}: {f} differs"


def _form_launches(kind):
    """launch counters of the forms of one kernel list: name -> count"""
    from rt_amd import abi
    shim = abi.load_shim()
    count, fn = {"query": (shim.rt_hip_query_kernel_count, shim.rt_hip_query_kernel_launches),
                 "trace": (shim.rt_hip_trace_kernel_count, shim.rt_hip_trace_kernel_launches),
                 "pixel": (shim.rt_hip_pixel_kernel_count, shim.rt_hip_pixel_kernel_launches),
                 "aov": (shim.rt_hip_aov_kernel_count, shim.rt_hip_aov_kernel_launches)}[kind]
    out = {}
    for k in range(count()):
        n = C.c_uint64(0)
        name = fn(k, C.byref(n)).decode()   # (first the call that fills n, then its value)
        out[name] = n.value
    return out


def _launched(kind, form, call):
    """runs call() and asserts that the launches it made were of `form` alone"""
    before = _form_launches(kind)
    res = call()
    after = _form_launches(kind)
    moved = {k: after[k] - before[k] for k in after if after[k] != before[k]}
    assert list(moved) == [form] and moved[form] >= 1, f"{kind}: launches {moved}, expected {form}"
    return res


def _stats(a):
    return dict(rays=int(a[0]), casts=int(a[1]), tests=int(a[2]), samples=int(a[3]))


def _samples_meet_the_reference(what, sc, got, ref, valid, S):
    """a radiance or pixel query against the compiled reference's own samples, as tests/test_gpu_trace.py and test_gpu_refine.py
    compare them: status, paths, casts and counters exactly, every sample inside trace_expected.value_bar (2^-40 |ref| without
    glass), radiance the reduction of the samples bit for bit"""
    import trace_expected as T
    assert (got["status"] == np.where(valid, 1, 2)).all(), what
    assert (got["paths"] == ref["paths"]).all() and (got["casts"] == ref["casts"]).all(), what
    assert _stats(got["stats"]) == dict(rays=int(ref["paths"].sum()), casts=int(ref["casts"].sum()),
                                        tests=int(ref["casts"].sum()) * sc.n_primitives, samples=int(valid.sum()) * S), what
    err, bar = np.abs(got["samples"] - ref["samples"]), T.value_bar(ref["samples"], False)
    ratio = float((err[bar > 0] / bar[bar > 0]).max()) if (bar > 0).any() else 0.0
    print(f"{what}: worst |got - ref| / bar = {ratio:.3e}")
    assert (err <= bar).all(), f"{what}: {(err > bar).sum()} sample values beyond the bar, worst ratio {ratio}"
    assert np.array_equal(got["radiance"].view(np.uint64), T.reduce_samples(got["samples"]).view(np.uint64)), what


@pytest.fixture(scope="module")
def query_pair(gpu):
    """the _tri_big class of the query tests (400 triangles next to 12 spheres, no back wall) at the frame tests' size and depth,
    built by the host and by the device"""
    sc = class_scene(**dict(dict(n_packed=4, tris=400, open_back=True), **FRAME))
    pair = dict(zip(("host", "device"), _pair(gpu, sc)))
    yield sc, pair
    for gs in pair.values():
        gs.close()
    sc.free()


def test_ray_queries_through_a_device_tree(query_pair, ref_mesh):
    """pt_query_rays_tri_big: the compiled reference's closest hits (query_expected) through either tree, and the same bits"""
    import query_expected as Q
    sc, pair = query_pair
    rays = Q.ray_set(sc)
    exp = Q.expected(ref_mesh(16), sc, rays=rays)
    got = {}
    for name, gs in pair.items():
        got[name] = _launched("query", "pt_query_rays_tri_big", lambda: _np(gs.query_rays(rays)))
        msg = Q.mismatch(got[name], exp)
        assert not msg, f"{name} tree: {msg}"
        assert gs.launch_status() == 0
    assert (got["device"]["prim"] != 0xFFFFFFFF).sum() > 20, "the rays must meet triangles"
    _same_bits(got["host"], got["device"], "query")


def test_radiance_queries_through_a_device_tree(query_pair, ref_mesh, pt):
    """pt_trace_rays_tri_big: 65 rays x 2 samples at depth 16 against the compiled reference's samples through either tree"""
    import trace_expected as T
    sc, pair = query_pair
    o, q = T.ray_set(sc, open_back=True)
    n, S = 65, 2
    ref = T.reference_samples(ref_mesh(16), sc, o[:n], q[:n], S, T.SEED, 0, casts_oracle=pt)
    got = {}
    for name, gs in pair.items():
        got[name] = _launched("trace", "pt_trace_rays_tri_big", lambda: _np(gs.trace_rays(
            ref["rays"], S, T.SEED, want=("status", "radiance", "samples", "paths", "casts", "ray"))))
        _samples_meet_the_reference(f"trace_rays {name} tree", sc, got[name], ref, np.ones(n, bool), S)
        assert np.array_equal(got[name]["ray"].view(np.uint64), ref["rays"].view(np.uint64)) and gs.launch_status() == 0
    _same_bits(got["host"], got["device"], "trace_rays")


def test_pixel_queries_through_a_device_tree(query_pair, ref_mesh, pt):
    """pt_trace_pixels_tri_big: render()'s samples 0 and 1 of refine_expected.pixel_list against the compiled reference"""
    import refine_expected as R
    sc, pair = query_pair
    pixels = R.pixel_list(sc.width, sc.height)
    valid = pixels < sc.width * sc.height
    ref = R.expected_pixels(ref_mesh(16), sc, pixels, 2, 0, R.SEED, casts_oracle=pt)
    got = {}
    for name, gs in pair.items():
        got[name] = _launched("pixel", "pt_trace_pixels_tri_big", lambda: _np(gs.trace_pixels(
            pixels, 2, R.SEED, want=("status", "radiance", "samples", "paths", "casts"))))
        assert (got[name]["status"] == ref["status"]).all()
        _samples_meet_the_reference(f"trace_pixels {name} tree", sc, got[name], ref, valid, 2)
        assert gs.launch_status() == 0
    _same_bits(got["host"], got["device"], "trace_pixels")


def test_first_hit_buffers_through_a_device_tree(query_pair, ref_mesh):
    """pt_aov_tiles_tri_big: the whole buffers equal the expectation built from the compiled reference (aov_expected) bit for bit"""
    import aov_expected as A
    sc, pair = query_pair
    exp = A.expected_image(ref_mesh(16), sc, SEED, 2)
    got = {}
    for name, gs in pair.items():
        got[name] = _launched("aov", "pt_aov_tiles_tri_big", lambda: gs.aov_image(SEED, 2))
        msg = A.mismatch(got[name], exp)
        assert not msg, f"{name} tree: {msg}"
        assert gs.launch_status() == 0
    for f in got["host"]:
        assert np.array_equal(np.asarray(got["host"][f]).view(np.uint8), np.asarray(got["device"][f]).view(np.uint8)), f


def test_duplicated_triangles_keep_the_first_index(gpu):
    """every triangle twice: equal t at every hit, and the lower index must win whatever order the leaves hold them in"""
    tris = M.mesh("duplicated") * 3.0
    sc = mesh_scene(tris)
    rays = np.zeros((len(tris), 6))
    rays[:, 3:] = tris.mean(axis=1)          # from the origin at every triangle's centroid, both copies of it
    got = []
    for gs in _pair(gpu, sc):
        got.append(_np(gs.query_rays(rays, normalize=True, want=("status", "t", "prim", "object"))))
        gs.close()
    prim = got[1]["prim"].view(np.uint32)
    hit = got[1]["object"].view(np.uint32) == 1
    assert hit.sum() >= 250 and (prim[hit] % 2 == 0).all(), "a hit on a doubled triangle reports the first of the two"
    _same_bits(got[0], got[1], "duplicated")


def test_skipping_rules_hold_on_a_device_tree():
    """one frame of the 10,240-triangle sphere through the PT_DIAG build with a device-built tree: the exhaustive re-checks of the
    conservative rules (filter, pre-tests, probe, hull facets) find nothing"""
    env = dict(os.environ, RT_HIP_SHIM_PATH=os.path.join(ROOT, "raytracer.c_amd", "csrc", "librt_hip_diag.so"))
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "bvh_device_diag_child.py")], env=env, capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    rec = json.loads(out.stdout.strip().splitlines()[-1])
    print(rec)
    assert rec["builder"] == "device" and rec["violations"] == 0
    assert rec["leaf_pretests"] > 0 and rec["casts"] > 0, "the check was not vacuous"


def test_c_host_builder_setter(gpu):
    """rt_hip_render_image under rt_hip_set_bvh_builder: the same frame, one rebuild per change -- also on three logical devices"""
    from rt_amd import abi
    shim = abi.load_shim()
    sc = class_scene(**dict(dict(n_packed=4, tris=400, round_mesh=True), **FRAME))
    assert shim.rt_hip_set_bvh_builder(0) == 0
    for map_, n_dev in ((None, 1), ((C.c_int * 3)(0, 0, 0), 3)):
        assert shim.rt_hip_set_device_map(map_, 3 if map_ is not None else 0) == 0
        assert shim.rt_hip_set_bvh_builder(0) == 0
        host = gpu.render_image_host(sc, SEED, n_devices=n_dev)
        b0 = shim.rt_hip_cache_builds()
        assert shim.rt_hip_set_bvh_builder(1) == 0
        dev = gpu.render_image_host(sc, SEED, n_devices=n_dev)
        assert shim.rt_hip_cache_builds() == b0 + 1, "a change of the builder rebuilds the cached context once"
        dev2 = gpu.render_image_host(sc, SEED, n_devices=n_dev)
        assert shim.rt_hip_cache_builds() == b0 + 1
        for other in (dev, dev2):
            assert np.array_equal(host[0], other[0]) and np.array_equal(host[1], other[1]) and host[2] == other[2]
    shim.rt_hip_set_bvh_builder(0)
    shim.rt_hip_set_device_map(None, 0)
    shim.rt_hip_release_cache()
    sc.free()


def test_cli_flag_writes_the_same_png(tmp_path):
    cli = os.path.join(ROOT, "raytracer.c_amd", "host", "raytracer")
    pngs = []
    for b in ("0", "1"):
        path = str(tmp_path / f"c5_b{b}.png")
        out = subprocess.run([cli, "-c", "5", "-w", "96", "-h", "54", "-s", "2", "-b", b, "-o", path], capture_output=True, text=True,
                             timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        pngs.append(open(path, "rb").read())
    assert pngs[0] == pngs[1] and len(pngs[0]) > 100
    bad = subprocess.run([cli, "-c", "5", "-b", "2"], capture_output=True, text=True, timeout=60)
    assert bad.returncode != 0 and "-b" in bad.stderr

"""A tree priced on the device and rebuilt in place (include/rt_hip.h: rt_hip_scene_bvh_cost, rt_hip_bvh_cost_nodes_host,
rt_hip_scene_rebuild_bvh, rt_hip_scene_maintain_bvh; raytracer.c_amd/csrc/scene_update.hip: k_tree_cost).

  1. the cost kernel equals the numpy restatement of its contract (tests/bvh_cost_expected.py) bit for bit: synthetic nodes at the
     block and level edges of the reduction (1, 2, 255, 256, 257, 65,535, 65,536, 65,537), the totality cases, a logical device,
     and a real scene's nodes;
  2. after update_vertices + rebuild_bvh a scene equals GpuScene(bvh="device") created from the moved positions: nodes and order
     byte for byte, bvh_info field for field, the triangle records, the kernel names, a frame (floats, bytes, counters) and a
     query_rays batch -- from host-built and device-built scenes, at 1, 15, 16, 17 and 3,000 triangles, and on the scene class
     whose launches walk the hierarchy (asserted by the kernels' names);
  3. node counts that grow and shrink (the committed pairs, which tests/test_bvh_rebuild_cpu.py shows to differ): rebuild, a
     second update (the level array is made again), a launch at another camera distance (an owned table set at the new size),
     rebuild back -- equal to the fresh scene at every step;
  4. refusals leave nodes, order and frame as they were;
  5. maintain_bvh: never above a huge ratio, once at 1.0 after a deformation that raises the cost, and then ratio 1 exactly;
  3b. one scene climbing through three trees of ever more nodes: a rebuild before the first launch, a side allocation replaced by a
     larger one;
  6b. the C host: render_ex in a loop under rt_set_scene_updates(1) and rt_set_bvh_rebuild_ratio;
  6. the cached context of rt_hip_render_image: frame A, a deformed B, A again under rt_hip_set_scene_updates(1) and a ratio --
     builds, updates and rebuilds counted (the rebuilds against a CPU run of the same decisions), frames equal to the uncached
     ones, also on 2 logical devices: the rebuild and the cost kernel on a logical device.
No existing allocation-failure hook covers the builder's workspace or the side allocation: those two refusals are not injected."""
import ctypes as C

import numpy as np
import pytest

import bvh_cost_expected as E
import bvh_sweep_meshes as M
import scene_update_meshes as U
from conftest import SEED
from test_gpu_scene_update import (as_input, assert_same_frame, assert_same_state, frame, mesh_scene, move_scene, state, tris_of)
from util import class_scene

pytestmark = pytest.mark.gpu
FRAME = dict(width=32, height=24, samples=4, depth=4)
HUGE_RATIO = 1e300


@pytest.fixture(scope="module")
def gpu():
    import torch
    from rt_amd import abi, gpu as G
    shim = abi.load_shim()
    assert shim.rt_hip_device_count() >= 1, "no HIP device: the GPU tests must run on the GPU box"
    assert torch.cuda.is_available()
    yield G
    shim.rt_hip_set_scene_updates(0)
    shim.rt_hip_set_bvh_rebuild_ratio(0.0)
    shim.rt_hip_set_bvh_builder(0)
    shim.rt_hip_set_device_map(None, 0)
    shim.rt_hip_release_cache()


def device_cost(nodes, device=0):
    from rt_amd import abi, gpu as G
    nodes = np.ascontiguousarray(nodes, dtype=np.float64)
    cost = C.c_double(-1.0)
    G._check(abi.load_shim().rt_hip_bvh_cost_nodes_host(nodes.ctypes.data if len(nodes) else None, len(nodes), device, C.byref(cost)),
             "rt_hip_bvh_cost_nodes_host")
    return cost.value


@pytest.mark.parametrize("n", E.EDGE_SIZES)
def test_cost_kernel_at_the_reduction_edges(gpu, n):
    nodes = E.synthetic_nodes(n)
    got, want = device_cost(nodes), E.cost(nodes)
    print(f"{n} nodes: device {got!r}, restatement {want!r}")
    assert np.isfinite(want) and want > 60.0
    assert E.same_cost(got, want), f"{n} nodes: device {got!r}, restatement {want!r}"
    assert E.same_cost(device_cost(nodes), got), "two runs over the same bytes differ"


def test_cost_kernel_totality(gpu):
    for name, nodes in E.totality_cases().items():
        got, want = device_cost(nodes), E.cost(nodes)
        print(f"{name}: device {got!r}, restatement {want!r}")
        assert E.same_cost(got, want), f"{name}: device {got!r}, restatement {want!r}"
    assert device_cost(np.zeros((0, 16))) == 0.0


def test_cost_on_a_logical_device(gpu):
    from rt_amd import abi
    shim = abi.load_shim()
    assert shim.rt_hip_set_device_map((C.c_int * 2)(0, 0), 2) == 0
    try:
        nodes = E.synthetic_nodes(257)
        assert E.same_cost(device_cost(nodes, device=1), E.cost(nodes))
        cost = C.c_double(0)
        assert shim.rt_hip_bvh_cost_nodes_host(nodes.ctypes.data, len(nodes), 2, C.byref(cost)) == abi.ENODEV   # the map has two entries
    finally:
        shim.rt_hip_set_device_map(None, 0)


def info_fields(gs):
    info = gs.bvh_info()
    info.pop("build_seconds")
    return info


def assert_same_tree(gs, fresh, what):
    """nodes and order byte for byte, bvh_info field for field (the device cost among them), records and kernel names"""
    (n1, o1), (n2, o2) = gs.bvh_read(), fresh.bvh_read()
    assert n1.shape == n2.shape, f"{what}: {len(n1)} nodes, the fresh scene {len(n2)}"
    assert np.array_equal(n1.view(np.uint64), n2.view(np.uint64)), f"{what}: nodes differ from the fresh scene's"
    assert np.array_equal(o1, o2), f"{what}: the leaf order differs from the fresh scene's"
    a, b = info_fields(gs), info_fields(fresh)
    assert a == b and a["builder"] == "device", f"{what}: bvh_info {a}, the fresh scene {b}"
    want = E.cost(n2)
    assert E.same_cost(gs.bvh_cost(), want) and E.same_cost(fresh.bvh_cost(), want), f"{what}: device cost {gs.bvh_cost()!r}, restatement {want!r}"
    assert_same_state(state(gs), state(fresh), what)


def query_bits(gs, rays):
    import torch
    out = gs.query_rays(rays)
    torch.cuda.synchronize()
    return {f: np.ascontiguousarray(t.cpu().numpy()).view(np.uint8) for f, t in out.items()}


def assert_same_launches(gs, fresh, rays, what, integrator="path"):
    got, exp = frame(gs, integrator), frame(fresh, integrator)
    assert_same_frame(got, exp, what)
    a, b = query_bits(gs, rays), query_bits(fresh, rays)
    assert gs.query_kernel_name() == fresh.query_kernel_name()
    for f in b:
        assert np.array_equal(a[f], b[f]), f"{what}: query field {f} differs from the fresh scene's"
    assert gs.launch_status() == 0
    return got


SIZES = {"n1": "n1", "n15": "n15", "n16": "n16", "n17": "n17", "n3000": "shell3000"}


@pytest.mark.parametrize("builder", ["host", "device"])
@pytest.mark.parametrize("name", list(SIZES))
def test_rebuild_equals_a_fresh_device_scene(gpu, name, builder):
    import query_expected as Q
    tris = np.array(M.mesh(SIZES[name])) * 3.0
    gs = gpu.GpuScene(mesh_scene(tris, **FRAME), bvh=builder)
    frame(gs)                                          # table set 0 exists before the first rebuild
    assert gs.rebuild_info()["rebuilds"] == 0
    for k, deform in enumerate(("scale_wobble", "mirror", "squash")):
        what = f"{name} {builder} {deform}"
        new = U.DEFORMATIONS[deform](tris)
        moved = mesh_scene(new, **FRAME)
        fresh = gpu.GpuScene(moved, bvh="device")
        gs.update_vertices(as_input(gpu, new, k))
        gs.rebuild_bvh()
        assert_same_tree(gs, fresh, what)
        assert_same_launches(gs, fresh, Q.ray_set(moved, 256), what)
        ri = gs.rebuild_info()
        assert ri["rebuilds"] == k + 1 and ri["last_seconds"] > 0 and E.same_cost(ri["built_cost"], gs.bvh_cost())
        assert gs.update_info()["updates"] == k + 1, "a rebuild is not an update"
        fresh.close()
    gs.close()


@pytest.mark.parametrize("builder", ["host", "device"])
def test_rebuild_under_the_hierarchy_walking_forms(gpu, builder):
    import query_expected as Q
    cls = dict(dict(n_packed=4, tris=400), **FRAME)
    base, moved = class_scene(**cls), class_scene(**cls)
    new = U.scale_wobble(tris_of(base))
    move_scene(moved, new)
    gs, fresh = gpu.GpuScene(base, bvh=builder), gpu.GpuScene(moved, bvh="device")
    frame(gs)
    gs.update_vertices(as_input(gpu, new, 0))
    gs.rebuild_bvh()
    assert_same_tree(gs, fresh, builder)
    rays = Q.ray_set(moved, 256)
    got = assert_same_launches(gs, fresh, rays, f"{builder} path")
    assert got[3] == "pt_render_tiles_tri_queued", got[3]
    got = assert_same_launches(gs, fresh, rays, f"{builder} whitted", integrator="whitted")
    assert got[3] == "pt_whitted_tiles_tri_big", got[3]
    assert gs.query_kernel_name() == "pt_query_rays_tri_big"
    assert (query_bits(gs, rays)["prim"].view(np.uint32) != 0xFFFFFFFF).sum() > 20, "the rays must meet triangles"
    for s in (gs, fresh):
        s.close()
    base.free()
    moved.free()


def far_camera(sc):
    """the scene's camera from twice as far: another near_R, so another table set"""
    from rt_amd import abi
    cam = abi.Camera()
    C.memmove(C.byref(cam), C.byref(sc.camera), C.sizeof(abi.Camera))
    for f in ("x", "y", "z"):
        setattr(cam.position, f, 2.0 * getattr(sc.camera.position, f))
    return cam


def tiles_of(gs, camera):
    import torch
    t, t8, st = gs.render_tiles(SEED, 0, 1, 12, camera=camera)
    torch.cuda.synchronize()
    assert gs.launch_status() == 0
    return t.cpu().numpy().view(np.uint32), t8.cpu().numpy(), st.cpu().numpy()


@pytest.mark.parametrize("builder", ["host", "device"])
@pytest.mark.parametrize("name", list(E.PAIRS))
def test_node_counts_that_grow_and_shrink(gpu, name, builder):
    import query_expected as Q
    a, b = E.pair(name)
    sa, sb = mesh_scene(a, **FRAME), mesh_scene(b, **FRAME)
    fresh = {"a": gpu.GpuScene(sa, bvh="device"), "b": gpu.GpuScene(sb, bvh="device")}
    na, nb = fresh["a"].bvh_info()["n_nodes"], fresh["b"].bvh_info()["n_nodes"]
    assert nb > na if name == "grows" else nb < na, (na, nb)
    rays = {"a": Q.ray_set(sa, 256), "b": Q.ray_set(sb, 256)}
    cam = far_camera(sa)
    gs = gpu.GpuScene(mesh_scene(a, **FRAME), bvh=builder)
    frame(gs)
    tiles_of(gs, cam)                                  # an owned table set of the first tree's size
    for k, to in enumerate(("b", "a", "b")):
        what = f"{name} {builder} step {k} -> {to}"
        pos = b if to == "b" else a
        gs.update_vertices(as_input(gpu, pos, k))
        gs.rebuild_bvh()
        assert_same_tree(gs, fresh[to], what)
        assert_same_launches(gs, fresh[to], rays[to], what)
        gs.update_vertices(as_input(gpu, pos, k + 1))  # the level array of the new topology: a refit that changes nothing
        assert_same_tree(gs, fresh[to], what + ", updated again")
        for x, y in zip(tiles_of(gs, cam), tiles_of(fresh[to], cam)):   # an owned table set at the new size
            assert np.array_equal(x, y), f"{what}: the far camera's tiles differ from the fresh scene's"
        assert_same_launches(gs, fresh[to], rays[to], what + ", after the far launch")
    assert gs.rebuild_info()["rebuilds"] == 3
    for s in (gs, fresh["a"], fresh["b"]):
        s.close()


@pytest.mark.parametrize("builder", ["host", "device"])
def test_a_side_allocation_replaced_by_a_larger_one(gpu, builder):
    """the committed climb (25 < 28 < 30 nodes, tests/test_bvh_rebuild_cpu.py): the first rebuild comes before the scene's first
    launch -- no table set exists yet -- and makes a side allocation, the second needs a larger one and frees the first; then
    back down, in place in the larger one"""
    import query_expected as Q
    sets = E.climb()
    gs = gpu.GpuScene(mesh_scene(sets[0], **FRAME), bvh=builder)
    counts = []
    for k, j in enumerate((1, 2, 0, 2)):
        what = f"climb {builder} step {k} -> set {j}"
        moved = mesh_scene(sets[j], **FRAME)
        fresh = gpu.GpuScene(moved, bvh="device")
        gs.update_vertices(as_input(gpu, sets[j], k))
        gs.rebuild_bvh()                                 # k == 0: before any launch of this scene
        assert_same_tree(gs, fresh, what)
        assert_same_launches(gs, fresh, Q.ray_set(moved, 256), what)
        for x, y in zip(tiles_of(gs, far_camera(moved)), tiles_of(fresh, far_camera(moved))):
            assert np.array_equal(x, y), f"{what}: the far camera's tiles differ from the fresh scene's"
        counts.append(fresh.bvh_info()["n_nodes"])
        fresh.close()
    assert counts[0] < counts[1] and counts[2] < counts[0] and counts[3] == counts[1], counts
    assert gs.rebuild_info()["rebuilds"] == 4
    gs.close()


def host_frames(host, scenes):
    """render_ex of the C host over `scenes`, one after another -> [(bytes, linear floats)]"""
    from rt_amd import abi
    depth, seed, out = host.rt_get_max_depth(), host.rt_get_seed(), []
    for sc in scenes:
        fb, lin = np.zeros((sc.height, sc.width, 3), dtype=np.uint8), np.zeros((sc.height, sc.width, 3), dtype=np.float32)
        opt = abi.Options()
        opt.width, opt.height, opt.samples = sc.width, sc.height, sc.samples
        host.rt_set_max_depth(sc.max_depth)
        host.rt_set_seed(SEED)
        host.render_ex(fb.ctypes.data, lin.ctypes.data, sc.objects, sc.n_objects, sc.meshes, sc.n_meshes, C.byref(sc.camera), C.byref(opt))
        out.append((fb, lin))
    host.rt_set_max_depth(depth)
    host.rt_set_seed(seed)
    return out


def test_c_host_rebuilds_the_cached_scene(gpu, tmp_path_factory):
    """the host library's render_ex in a loop over A, a deformed B, A under rt_set_scene_updates(1) and rt_set_bvh_rebuild_ratio:
    one build, two updates, the rebuilds a CPU run of the same decisions expects, and the frames of fresh contexts"""
    from rt_amd import abi
    shim, host = abi.load_shim(), abi.load_host()
    refit = U.Refit(U.compile_harness(tmp_path_factory.mktemp("refit")))
    cls = dict(dict(n_packed=4, tris=400), **FRAME)
    a, b = class_scene(**cls), class_scene(**cls)
    move_scene(b, U.squash(U.mirror(tris_of(a))))
    sequence = [tris_of(a), tris_of(b), tris_of(a)]
    try:
        host.rt_set_bvh_builder(0)                        # the scenes of the cached context: host-built, as `expected` assumes
        host.rt_set_scene_updates(0)
        host.rt_set_bvh_rebuild_ratio(0.0)
        want = []
        for sc in (a, b, a):                              # every frame from a context of its own
            shim.rt_hip_release_cache()
            want += host_frames(host, [sc])
        for ratio in (1.0, 0.0):
            expected = expected_rebuilds(refit, "host", sequence, ratio)
            assert expected >= 1 if ratio else expected == 0
            shim.rt_hip_release_cache()
            host.rt_set_scene_updates(1)
            host.rt_set_bvh_rebuild_ratio(ratio)
            assert host.rt_get_bvh_rebuild_ratio() == ratio
            c0 = (shim.rt_hip_cache_builds(), shim.rt_hip_cache_updates(), shim.rt_hip_cache_rebuilds())
            got = host_frames(host, [a, b, a])
            c1 = (shim.rt_hip_cache_builds(), shim.rt_hip_cache_updates(), shim.rt_hip_cache_rebuilds())
            assert tuple(y - x for x, y in zip(c0, c1)) == (1, 2, expected), f"ratio {ratio}: {c0} -> {c1}, {expected} rebuilds expected"
            for (fb, lin), (wfb, wlin) in zip(got, want):
                assert np.array_equal(fb, wfb) and np.array_equal(lin.view(np.uint32), wlin.view(np.uint32))
    finally:
        host.rt_set_scene_updates(0)
        host.rt_set_bvh_rebuild_ratio(0.0)
        shim.rt_hip_release_cache()
        a.free()
        b.free()


def test_refusals_leave_the_scene_alone(gpu):
    from rt_amd import abi
    tris = np.array(M.mesh("n257")) * 3.0
    gs = gpu.GpuScene(mesh_scene(tris, **FRAME), bvh="host")
    gs.update_vertices(U.scale_wobble(tris))
    (n0, o0), f0, i0 = gs.bvh_read(), frame(gs), info_fields(gs)

    def refused(scene, call, code, word):
        with pytest.raises(gpu.ShimError) as e:
            call()
        assert f"({code})" in str(e.value) and word in str(e.value), str(e.value)
        n1, o1 = gs.bvh_read()
        assert np.array_equal(n1.view(np.uint64), n0.view(np.uint64)) and np.array_equal(o1, o0), f"{word}: the tree changed"
        assert info_fields(gs) == i0 and gs.rebuild_info()["rebuilds"] == 0
        assert_same_frame(frame(gs), f0, word)

    assert gs.maintain_bvh(HUGE_RATIO)["cost_ratio"] > 1.0, "the refitted tree must be dearer, or maintain_bvh(1.0) asks for nothing"
    acc = gs.accumulate(SEED, 4)
    refused(gs, gs.rebuild_bvh, abi.EINVAL, "accumulation")
    refused(gs, lambda: gs.maintain_bvh(1.0), abi.EINVAL, "accumulation")      # the refitted tree is dearer: it asks for the rebuild
    acc.close()
    refused(gs, lambda: gs.maintain_bvh(float("nan")), abi.EINVAL, "max_ratio")
    refused(gs, lambda: gs.maintain_bvh(0.999), abi.EINVAL, "max_ratio")
    balls = gpu.GpuScene(class_scene(n_packed=4, **FRAME))
    fb = frame(balls)
    for call in (balls.rebuild_bvh, lambda: balls.maintain_bvh(2.0)):
        with pytest.raises(gpu.ShimError) as e:
            call()
        assert f"({abi.EINVAL})" in str(e.value) and "no triangles" in str(e.value)
    assert balls.bvh_cost() == 0.0 and balls.rebuild_info() == {"rebuilds": 0, "last_seconds": 0.0, "built_cost": 0.0}
    assert_same_frame(frame(balls), fb, "a scene without triangles")
    balls.close()
    # and once nothing stands in the way, the rebuild goes through
    gs.rebuild_bvh()
    fresh = gpu.GpuScene(mesh_scene(U.scale_wobble(tris), **FRAME), bvh="device")
    assert_same_tree(gs, fresh, "after the refusals")
    assert_same_frame(frame(gs), frame(fresh), "after the refusals")
    fresh.close()
    gs.close()


def test_maintain_bvh(gpu, tmp_path_factory):
    refit = U.Refit(U.compile_harness(tmp_path_factory.mktemp("refit")))
    tris = np.array(M.mesh("shell3000")) * 3.0
    new = U.scale_wobble(tris)
    # on the CPU: the tree as built, refitted to the deformed mesh, and its cost ratio by the restatement
    nodes, order = refit.build("device", M.geom(tris))
    refitted = refit.refit(nodes, order, M.geom(new))
    want = E.cost(refitted) / E.cost(nodes)
    print(f"cost as built {E.cost(nodes)!r}, refitted {E.cost(refitted)!r}, ratio {want!r}")
    assert want > 1.0, "the deformation must make the refitted tree dearer"
    gs = gpu.GpuScene(mesh_scene(tris, **FRAME), bvh="device")
    assert gs.maintain_bvh(HUGE_RATIO) == {"cost_ratio": 1.0, "rebuilt": False}
    assert gs.update_vertices(new) is None
    r = gs.maintain_bvh(HUGE_RATIO)
    assert r["rebuilt"] is False and E.same_cost(r["cost_ratio"], want), (r, want)
    assert E.same_cost(gs.rebuild_info()["built_cost"], E.cost(nodes)) and gs.rebuild_info()["rebuilds"] == 0
    r = gs.maintain_bvh(1.0)
    assert r["rebuilt"] is True and E.same_cost(r["cost_ratio"], want), (r, want)
    assert gs.maintain_bvh(1.0) == {"cost_ratio": 1.0, "rebuilt": False}
    assert gs.rebuild_info()["rebuilds"] == 1
    fresh = gpu.GpuScene(mesh_scene(new, **FRAME), bvh="device")
    assert_same_tree(gs, fresh, "maintained")
    assert_same_frame(frame(gs), frame(fresh), "maintained")
    # update_vertices(rebuild_above=...): the same decision in one call
    r = gs.update_vertices(tris, rebuild_above=HUGE_RATIO)
    assert r["rebuilt"] is False and r["cost_ratio"] != 1.0
    r = gs.update_vertices(tris, rebuild_above=1.0)
    assert r["rebuilt"] == (r["cost_ratio"] > 1.0)
    fresh.close()
    gs.close()


def expected_rebuilds(refit, builder, sequence, max_ratio):
    """what the cached context does, on the CPU: the tree of `builder` over sequence[0], then for every later position set a
    refit, the restatement's cost ratio against the tree as last built, and BvhSweep's tree where it is above max_ratio"""
    nodes, order = refit.build(builder, M.geom(sequence[0]))
    built, count = E.cost(nodes), 0
    for pos in sequence[1:]:
        nodes = refit.refit(nodes, order, M.geom(pos))
        if max_ratio and E.cost(nodes) / built > max_ratio:
            nodes, order = refit.build("device", M.geom(pos))
            built, count = E.cost(nodes), count + 1
    return count


def test_cached_context_rebuilds(gpu, tmp_path_factory):
    """rt_hip_render_image: frame A, a deformed B, A again, under rt_hip_set_scene_updates(1) and a rebuild ratio"""
    from rt_amd import abi
    shim = abi.load_shim()
    refit = U.Refit(U.compile_harness(tmp_path_factory.mktemp("refit")))
    cls = dict(dict(n_packed=4, tris=400), **FRAME)
    a, b = class_scene(**cls), class_scene(**cls)
    move_scene(b, U.squash(U.mirror(tris_of(a))))
    sequence = [tris_of(a), tris_of(b), tris_of(a)]
    for map_, n_dev in ((None, 1), ((C.c_int * 2)(0, 0), 2)):
        assert shim.rt_hip_set_device_map(map_, 2 if map_ is not None else 0) == 0
        for builder in (0, 1):
            assert shim.rt_hip_set_bvh_builder(builder) == 0
            shim.rt_hip_set_scene_updates(0)
            assert shim.rt_hip_set_bvh_rebuild_ratio(0.0) == 0
            want = {}
            for k, sc in (("a", a), ("b", b)):           # uncached: a fresh context each
                shim.rt_hip_release_cache()
                want[k] = gpu.render_image_host(sc, SEED, n_devices=n_dev)
            for ratio in (1.0, HUGE_RATIO, 0.0):
                rebuilds = expected_rebuilds(refit, "device" if builder else "host", sequence, ratio)
                assert rebuilds >= 1 if ratio == 1.0 else rebuilds == 0, "the deformation must make the refitted tree dearer"
                shim.rt_hip_release_cache()
                shim.rt_hip_set_scene_updates(1)
                assert shim.rt_hip_set_bvh_rebuild_ratio(ratio) == 0
                c0 = (shim.rt_hip_cache_builds(), shim.rt_hip_cache_updates(), shim.rt_hip_cache_rebuilds())
                got = [gpu.render_image_host(sc, SEED, n_devices=n_dev) for sc in (a, b, a)]
                c1 = (shim.rt_hip_cache_builds(), shim.rt_hip_cache_updates(), shim.rt_hip_cache_rebuilds())
                counts = tuple(y - x for x, y in zip(c0, c1))
                assert counts == (1, 2, rebuilds), f"{n_dev} devices, builder {builder}, ratio {ratio}: {counts}, {rebuilds} rebuilds expected"
                for other, k in zip(got, ("a", "b", "a")):
                    assert np.array_equal(want[k][0].view(np.uint32), other[0].view(np.uint32)) and np.array_equal(want[k][1], other[1])
                    assert want[k][2] == other[2]
    shim.rt_hip_set_scene_updates(0)
    shim.rt_hip_set_bvh_rebuild_ratio(0.0)
    shim.rt_hip_set_bvh_builder(0)
    shim.rt_hip_set_device_map(None, 0)
    shim.rt_hip_release_cache()
    a.free()
    b.free()

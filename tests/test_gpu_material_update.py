"""Materials edited in place: GpuScene.update_materials (rt_hip_scene_update_materials, raytracer.c_amd/csrc/scene_update.hip:
k_update_materials).

The contract: after an update the records (read_materials: a NaN equal to a NaN, every other word by its bits), the scalars a scene
derives from its materials (material_bounds), the kernel names of every integrator and of the query, trace, pixel and AOV forms,
and the frames, bytes and counters of every launch equal a scene freshly created from the same data.
  1. per scene -- one for every way materials reach a kernel (SCENES) -- a chain of steps from M0 and back to it (STEPS): a wall
     recoloured and the lamps dimmed with flags=None; every emission 0 (max_emission 0); a lamp at 1e9 (the accumulation's scale
     moves); a sphere to mirror, to glass, to mirror and glass; a checkered wall; a glass mesh and a checkered mesh.  After every
     step: state, "path" and "whitted" frames, first-hit buffers (the albedo reads color_raw) and probe_preview (k_probe_emission
     reads the records) against the fresh scene's, and the fresh frame differs from M0's;
  2. ray queries give the same outputs before and after an update;
  3. device tensors (a non-contiguous one among them) and numpy arrays give the same result, and materials() follows;
  4. every refusal leaves records and scalars as they were;
  5. a ProbeGridState on the room: after an update of the lamp, reset() and one update() is the grid bake of a fresh scene of the
     new materials; without the reset rounds run and every status word stays 1;
  6. the cached context under rt_hip_set_material_updates: (builds, updates) = (1, 1) when on, (2, 0) when off, on 1 and on 2
     logical devices, frames equal to a fresh context's; with a sphere move in the same call and rt_set_scene_updates(1) one build;
     and chunked frames (256 spp) across a ball turned to glass and a checkered wall: the context's chunk workspace follows the
     flag class;
  7. the host library under rt_set_probe_update: a changed emission runs a round when the switch is on, the full bake when off.
"""
import ctypes as C
import os

import numpy as np
import pytest

import material_expected as E
import probe_update_expected as PU
from conftest import SEED
from test_gpu_scene_update import assert_same_frame, frame
from util import class_scene

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WALL, BALL, BALL2 = 0, 6, 11      # class_scene: six walls, a diffuse ball and a mirror, then the packed spheres (some of them lamps)


def cube_tris():
    verts, tris = [], []
    for line in open(os.path.join(ROOT, "tests", "golden", "c3_cube.obj")):      # config 3's cube: 12 triangles
        part = line.split()
        if part and part[0] == "v":
            verts.append([float(t) for t in part[1:4]])
        elif part and part[0] == "f":
            idx = [int(t.split("/")[0]) - 1 for t in part[1:]]
            tris += [[verts[idx[0]], verts[idx[k]], verts[idx[k + 1]]] for k in range(1, len(idx) - 1)]
    return np.array(tris, np.float64) * 6.0 + np.array([3.0, -2.0, 10.0])


def cube_scene():
    """the room's spheres and the cube: the mesh's material sits at n_spheres + 0"""
    from rt_amd import abi, scene as S
    room = class_scene(n_packed=4)
    objs = [dict(flags=int(room.objects[i].flags), radius=float(room.objects[i].radius), center=room.objects[i].center.tuple(),
                 color=room.objects[i].color.tuple(), emission=room.objects[i].emission.tuple()) for i in range(room.n_objects)]
    room.free()
    return S.custom_scene(objs, 48, 32, 3, 5, (0, 0, 50), (0, 0, 0), meshes=[dict(flags=abi.M_DEFAULT, color=(0.7, 0.8, 0.9), triangles=cube_tris())])


SCENES = {
    "room": lambda: class_scene(n_packed=4),                              # staged in LDS per launch
    "spheres100": lambda: class_scene(n_packed=92),                       # 100 spheres: streamed (above PT_STREAM_ABOVE_BYTES)
    "spheres300": lambda: class_scene(n_packed=292),                      # 300 spheres: beyond the LDS budget, the _mem forms
    "cube": cube_scene,                                                   # the flat _tri form, a mesh's material
    "mesh400": lambda: class_scene(n_packed=4, tris=400, round_mesh=True),   # the hierarchy
}


def lamps(emission):
    return np.flatnonzero(np.abs(emission).max(axis=1) > 0)


def steps(sc):
    """-> [(name, colors, emission, flags or None: the flags stay)] from the scene's own materials M0, each step M0 but for what
    its name says; the last is M0 again"""
    c0, e0, f0 = E.materials_of(sc)
    n_sph, lit = sc.n_objects, lamps(E.materials_of(sc)[1])
    assert len(lit) >= 1 and f0[BALL] == E.M_DEFAULT and BALL not in lit
    out = []

    def step(name, flags_given=True):
        c, e, f = c0.copy(), e0.copy(), f0.copy()
        out.append([name, c, e, f, flags_given])
        return c, e, f
    c, e, f = step("recoloured wall, dimmed lamps, flags=None", flags_given=False)
    c[WALL] = (0.1, 0.9, 0.3)
    e[lit] *= 0.25
    c, e, f = step("lamps off")
    e[:] = 0.0
    c, e, f = step("a lamp at 1e9")
    e[lit[0]] = (1e9, 0.5e9, 1e9)
    c, e, f = step("a sphere to mirror")
    f[BALL], e[BALL] = E.M_REFLECTION, 0.0
    c, e, f = step("a sphere to glass")
    f[BALL], e[BALL], c[BALL] = E.M_REFRACTION, 0.0, (0.95, 0.95, 0.95)
    c, e, f = step("a sphere to mirror and glass")
    f[BALL2], e[BALL2] = E.M_REFLECTION | E.M_REFRACTION, 0.0
    c, e, f = step("a checkered wall")
    f[WALL] |= E.M_CHECKERED
    if sc.n_meshes:
        c, e, f = step("a glass mesh")
        f[n_sph], c[n_sph] = E.M_REFRACTION, (0.9, 0.9, 0.9)
        c, e, f = step("a checkered mesh")
        f[n_sph] |= E.M_CHECKERED
        c[n_sph] = (0.2, 0.3, 0.9)
    step("M0 again")
    return out


@pytest.fixture(scope="module")
def gpu():
    import torch
    from rt_amd import abi, gpu as G
    assert abi.load_shim().rt_hip_device_count() >= 1, "no HIP device: the GPU tests must run on the GPU box"
    assert torch.cuda.is_available()
    yield G
    abi.load_host().rt_set_material_updates(0)
    abi.load_host().rt_set_scene_updates(0)
    abi.load_shim().rt_hip_set_device_map(None, 0)


def state(gs):
    s = gs.read_materials()
    s.update(bounds=gs.material_bounds(), kernels={k: gs.kernel_name(k) for k in ("path", "whitted")})
    s["kernels"].update(query=gs.query_kernel_name(), trace=gs.trace_kernel_name(), pixel=gs.pixel_kernel_name(), aov=gs.aov_kernel_name())
    return s


def assert_same_state(got, want, what):
    for f in ("material", "color_raw"):
        assert E.same_records(got[f], want[f]), f"{what}: {f} differs from the fresh scene's"
    gb, wb = got["bounds"], want["bounds"]
    assert E.same_bits(gb["max_emission"], wb["max_emission"]), f"{what}: max_emission {gb['max_emission']!r} != {wb['max_emission']!r}"
    assert gb == wb or np.isnan(gb["max_emission"]), f"{what}: {gb} != {wb}"
    assert got["kernels"] == want["kernels"], f"{what}: {got['kernels']} != {want['kernels']}"


def probe_grid(gs):
    from rt_amd import abi
    r = gs.bounds()["reach"]
    return abi.probe_grid([-r] * 3, [2.0 * r] * 3, (2, 2, 2))


def outputs(gs, coeff):
    """everything a launch gives that a material decides: two frames, the first-hit buffers, the probe-lit preview"""
    import torch
    out = dict(path=frame(gs), whitted=frame(gs, "whitted"))
    out["aov"] = {f: np.ascontiguousarray(x).view(np.uint8) for f, x in gs.aov_image(SEED, 2).items()}
    rgb, rgb8 = gs.probe_preview(probe_grid(gs), coeff, seed=SEED)
    torch.cuda.synchronize()
    out["preview"] = (rgb.cpu().numpy().view(np.uint32), rgb8.cpu().numpy())
    assert gs.launch_status() == 0
    return out


def assert_same_outputs(got, want, what):
    for integrator in ("path", "whitted"):
        assert_same_frame(got[integrator], want[integrator], f"{what}, {integrator}")
    assert got["aov"].keys() == want["aov"].keys() and "albedo" in got["aov"]
    for f in got["aov"]:
        assert np.array_equal(got["aov"][f], want["aov"][f]), f"{what}: first-hit buffer {f} differs from the fresh scene's"
    for a, b in zip(got["preview"], want["preview"]):
        assert np.array_equal(a, b), f"{what}: the probe-lit preview differs from the fresh scene's"


def differs(a, b):
    return not np.array_equal(a["path"][0].view(np.uint32), b["path"][0].view(np.uint32))


def as_input(x, k):
    """a device tensor (even k: the device entry) or a numpy array (odd k: the host entry)"""
    import torch
    if x is None:
        return None
    if k % 2:
        return np.ascontiguousarray(x)
    return torch.tensor(x.astype(np.int32) if x.dtype == np.uint32 else x, device="cuda")


@pytest.mark.parametrize("name", list(SCENES))
def test_update_equals_a_fresh_scene(gpu, name):
    import torch
    base = SCENES[name]()
    chain = steps(base)
    coeff = torch.from_numpy(np.random.default_rng(5).uniform(0.0, 0.6, (8, 9, 3))).cuda()
    gs = gpu.GpuScene(base)
    st0, out0 = state(gs), outputs(gs, coeff)
    c0, e0, f0 = E.materials_of(base)
    want0 = E.expected(np.concatenate([c0, e0], axis=1), f0)
    assert E.same_records(st0["material"], want0["material"]), f"{name}: a created scene's records against the scalar restatement"
    assert st0["bounds"]["max_emission"] == want0["max_emission"] and not st0["bounds"]["any_refract"]
    kernels = set()
    for k, (step, c, e, f, flags_given) in enumerate(chain):
        what = f"{name}: {step}"
        gs.update_materials(as_input(c, k), as_input(e, k), as_input(f, k) if flags_given else None)
        other = SCENES[name]()
        E.set_materials(other, c, e, f)
        fresh = gpu.GpuScene(other)
        got_state, want_state = state(gs), state(fresh)
        assert_same_state(got_state, want_state, what)
        want = E.expected(np.concatenate([c, e], axis=1), f)
        assert E.same_records(got_state["material"], want["material"]) and E.same_records(got_state["color_raw"], want["color_raw"]), what
        b = got_state["bounds"]
        assert b["max_emission"] == want["max_emission"], what
        assert (b["any_refract"], b["any_checker"], b["any_mirror_glass"]) == tuple(bool(want["classes"] & bit) for bit in (1, 2, 4)), what
        got, exp = outputs(gs, coeff), outputs(fresh, coeff)
        assert_same_outputs(got, exp, what)
        kernels.add((got_state["kernels"]["path"], got_state["kernels"]["whitted"]))
        if step == "M0 again":
            assert_same_state(got_state, st0, what + " against the state before any update")
            assert_same_outputs(got, out0, what + " against the outputs before any update")
        else:
            assert differs(exp, out0), f"{what}: the fresh frame equals M0's: the update would show nothing"
        if step == "lamps off":
            assert b["max_emission"] == 0.0
        if step == "a lamp at 1e9":
            assert b["max_emission"] == 1e9
        if step == "a sphere to glass":
            assert b["any_refract"] and got_state["kernels"]["path"] != st0["kernels"]["path"], what
        if step == "a sphere to mirror and glass":
            # (two children a hit under cast_ray: the general in-memory kernel, which spheres300 is on already)
            assert b["any_mirror_glass"] and got_state["kernels"]["whitted"] == "pt_whitted_tiles_mem", what
            assert name == "spheres300" or st0["kernels"]["whitted"] != "pt_whitted_tiles_mem", what
        if step in ("a checkered wall", "a checkered mesh"):
            assert b["any_checker"] and got_state["kernels"]["aov"] != st0["kernels"]["aov"], what
        fresh.close()
        other.free()
    assert gs.update_info()["updates"] == len(chain) and gs.update_info()["last_seconds"] > 0
    assert len(kernels) >= 3, kernels
    gs.close()
    base.free()


def test_ray_queries_are_unaffected(gpu):
    import query_expected as Q
    import torch
    base = SCENES["cube"]()
    gs = gpu.GpuScene(base)
    rays = Q.ray_set(base)

    def ask():
        out = gs.query_rays(rays)
        torch.cuda.synchronize()
        return {f: np.ascontiguousarray(t.cpu().numpy()).view(np.uint8) for f, t in out.items()}
    before = ask()
    assert (before["status"].view(np.uint32) == 1).sum() > 20, "the rays must meet something"
    for _, c, e, f, _ in steps(base)[4:9]:
        gs.update_materials(c, e, f)
        after = ask()
        assert before.keys() == after.keys() and all(np.array_equal(before[k], after[k]) for k in before)
    gs.close()
    base.free()


def test_device_and_host_forms_give_the_same_result(gpu):
    import torch
    base = SCENES["spheres100"]()
    _, c, e, f, _ = steps(base)[4]
    a, b, d = gpu.GpuScene(base), gpu.GpuScene(base), gpu.GpuScene(base)
    tc, te = torch.tensor(c, device="cuda"), torch.tensor(e, device="cuda")
    tf = torch.tensor(f.astype(np.int32), device="cuda")
    a.update_materials(tc * 1.0, te, tf)                       # a tensor another kernel has just written on torch's stream
    b.update_materials(c, e, f)
    wide = torch.zeros((len(c), 6), dtype=torch.float64, device="cuda")
    wide[:, ::2] = tc
    assert not wide[:, ::2].is_contiguous()
    d.update_materials(wide[:, ::2], e, tf)                    # a non-contiguous tensor, and tensors mixed with arrays
    for other, what in ((b, "host form"), (d, "non-contiguous and mixed")):
        assert_same_state(state(a), state(other), f"device form against {what}")
        assert_same_frame(frame(a), frame(other), f"device form against {what}")
    for s in (a, b, d):
        mc, me, mf = s.materials()
        assert torch.equal(mc, tc) and torch.equal(me, te) and torch.equal(mf, tf), "materials(): the current ones"
    # uint32 flag tensors are taken as int32 ones are
    d.update_materials(tc, te, tf.view(torch.uint32))
    assert_same_state(state(a), state(d), "uint32 flags")
    assert d.materials()[2].dtype == torch.int32 and torch.equal(d.materials()[2], tf)
    # an omitted part keeps its current values
    a.update_materials(emission=e * 0.5)
    b.update_materials(c, e * 0.5, f)
    assert_same_state(state(a), state(b), "emission alone")
    with pytest.raises(ValueError):
        a.update_materials(colors=c[:-1])
    with pytest.raises(ValueError):
        a.update_materials(flags=f.astype(np.int64))
    for s in (a, b, d):
        s.close()
    base.free()


def test_refusals_leave_the_scene_alone(gpu):
    import torch
    from rt_amd import abi
    shim = abi.load_shim()
    base = SCENES["cube"]()
    c0, e0, f0 = E.materials_of(base)
    n = len(c0)
    gs = gpu.GpuScene(base)
    st0, f_before = state(gs), frame(gs)
    _, c, e, f, _ = steps(base)[0]
    new = np.ascontiguousarray(np.concatenate([c, e], axis=1))
    dev = torch.tensor(new, device="cuda")

    def refused(call, word, code=abi.EINVAL):
        with pytest.raises(gpu.ShimError) as err:
            call()
        assert f"({code})" in str(err.value) and word in str(err.value), str(err.value)
        assert_same_state(state(gs), st0, word)
        assert gs.update_info()["updates"] == 0

    host_form, dev_form = shim.rt_hip_scene_update_materials_host, shim.rt_hip_scene_update_materials
    refused(lambda: gpu._check(host_form(gs.handle, new.ctypes.data, None, n - 1), "update"), "count")
    refused(lambda: gpu._check(dev_form(gs.handle, C.c_void_p(dev.data_ptr()), None, n + 1), "update"), "count")
    refused(lambda: gpu._check(host_form(gs.handle, None, None, n), "update"), "required")
    refused(lambda: gpu._check(dev_form(gs.handle, None, None, n), "update"), "required")
    for bad_c, bad_e in (((-0.25, 0.5, 0.5), None), ((0.5, np.nan, 0.5), None), (None, (0.0, 2e100, 0.0)), (None, (0.0, 0.0, -2e100)),
                         ((0.5, 0.5, np.inf), None), (None, (np.nan, 0.0, 0.0))):
        bc, be = c.copy(), e.copy()
        if bad_c:
            bc[n - 2] = bad_c
        if bad_e:
            be[3] = bad_e
        refused(lambda: gs.update_materials(bc, be), "refused")                                              # the host entry
        refused(lambda: gs.update_materials(torch.tensor(bc, device="cuda"), torch.tensor(be, device="cuda")), "refused")
    acc = gs.accumulate(SEED, 4)
    refused(lambda: gs.update_materials(c, e), "accumulation")
    acc.close()
    refused(lambda: gs.update_materials(torch.tensor(c), torch.tensor(e)), "device memory")             # host tensors at the device entry
    host_flags = torch.tensor(f.astype(np.int32))
    refused(lambda: gpu._check(dev_form(gs.handle, C.c_void_p(dev.data_ptr()), C.c_void_p(host_flags.data_ptr()), n), "update"), "d_flags")
    inside, size = C.c_void_p(), C.c_size_t()
    assert shim.rt_hip_scene_memory(gs.handle, C.byref(inside), C.byref(size)) == 0 and size.value > 48 * n + 512
    refused(lambda: gpu._check(dev_form(gs.handle, C.c_void_p(inside.value + 256), None, n), "update"), "inside the scene")
    refused(lambda: gpu._check(dev_form(gs.handle, C.c_void_p(dev.data_ptr()), C.c_void_p(inside.value + size.value - 4 * n), n), "update"),
            "inside the scene")
    assert_same_frame(frame(gs), f_before, "after the refusals")
    # what rt_hip_scene_create accepts is accepted: a colour of -0.0 and an emission at the limit, once nothing stands in the way
    c[n - 2], e[3] = (-0.0, 0.5, 0.25), (1e100, 0.0, -1e100)
    gs.update_materials(c, e)
    other = SCENES["cube"]()
    E.set_materials(other, c, e, f0)
    fresh = gpu.GpuScene(other)
    assert_same_state(state(gs), state(fresh), "after the refusals")
    assert gs.material_bounds()["max_emission"] == 1e100 and gs.update_info()["updates"] == 1
    for s in (gs, fresh):
        s.close()
    # a scene without objects
    from rt_amd import scene as S
    empty = gpu.GpuScene(S.custom_scene([], 48, 32, 3, 5, (0, 0, 4), (0, 0, 0)))
    for rc in (dev_form(empty.handle, C.c_void_p(dev.data_ptr()), None, 0), host_form(empty.handle, new.ctypes.data, None, 1)):
        assert rc == abi.EINVAL and b"no objects" in shim.rt_hip_last_error()
    empty.close()
    for s in (base, other):
        s.free()


def test_probe_state_across_a_material_update(gpu):
    import torch
    samples, seed = 8, 77
    base = SCENES["room"]()
    c0, e0, f0 = E.materials_of(base)
    e1 = e0.copy()
    e1[lamps(e0)] = e1[lamps(e0)] * 3.0 + 1.0
    gs = gpu.GpuScene(base)
    grid = probe_grid(gs)
    ps = gs.probe_grid_state(grid, samples, seed, stride=1)
    ps.update(2)
    gs.update_materials(emission=e1)
    ps.update(3)                                                  # without a reset rounds run on the kept state
    torch.cuda.synchronize()
    assert ps.round == 5 and (ps.age.cpu().numpy() == 5).all() and (ps.status.cpu().numpy() == 1).all()
    ps.reset().update()
    other = SCENES["room"]()
    E.set_materials(other, c0, e1, f0)
    fresh = gpu.GpuScene(other)
    bake = fresh.bake_probe_grid(grid, samples, PU.round_seed(seed, 5))
    old = gs.bake_probe_grid(grid, samples, PU.round_seed(seed, 5))   # (the same scene by now)
    before = gpu.GpuScene(base).bake_probe_grid(grid, samples, PU.round_seed(seed, 5))
    torch.cuda.synchronize()
    got, want = ps.coeff.cpu().numpy(), bake.cpu().numpy()
    assert E.same_records(got, want), "reset() and one update() is the grid bake of a fresh scene of the new materials"
    assert E.same_records(old.cpu().numpy(), want) and not E.same_records(before.cpu().numpy(), want), "the new lamp shows in the bake"
    assert (ps.age.cpu().numpy() == 1).all() and (ps.status.cpu().numpy() == 1).all()
    for s in (gs, fresh):
        s.close()
    for s in (base, other):
        s.free()


def test_cached_context_updates_materials_in_place(gpu):
    """rt_hip_render_image under rt_hip_set_material_updates: a recoloured scene updates the cached context in place (one build, one
    update), also on 2 logical devices; with the default 0 the second call rebuilds; with a sphere move in the same call it takes
    both switches"""
    import sphere_update_expected as SE
    from rt_amd import abi
    shim, host = abi.load_shim(), abi.load_host()
    make = SCENES["mesh400"]
    base = make()
    _, c, e, f, _ = steps(base)[0]
    c[base.n_objects] = (0.3, 0.2, 0.8)                              # the mesh too
    f[BALL] = E.M_REFLECTION
    recoloured = make()
    E.set_materials(recoloured, c, e, f)
    moved_too = make()
    E.set_materials(moved_too, c, e, f)
    SE.move_scene(moved_too, SE.jitter(SE.spheres_of(base)))
    for map_, n_dev in ((None, 1), ((C.c_int * 2)(0, 0), 2)):
        assert shim.rt_hip_set_device_map(map_, 2 if map_ is not None else 0) == 0
        for other, moves, what in ((recoloured, 0, "materials"), (moved_too, 1, "materials and spheres")):
            host.rt_set_material_updates(0)
            host.rt_set_scene_updates(0)
            shim.rt_hip_release_cache()
            want = gpu.render_image_host(other, SEED, n_devices=n_dev)           # a fresh context for the changed scene
            first = gpu.render_image_host(base, SEED, n_devices=n_dev)
            assert not np.array_equal(want[0], first[0]), "the change must show"
            for mat_on, move_on in ((1, 1), (1, 0), (0, 1), (0, 0)):
                host.rt_set_material_updates(mat_on)
                host.rt_set_scene_updates(move_on)
                shim.rt_hip_release_cache()
                b0, u0 = shim.rt_hip_cache_builds(), shim.rt_hip_cache_updates()
                gpu.render_image_host(base, SEED, n_devices=n_dev)
                got = gpu.render_image_host(other, SEED, n_devices=n_dev)
                again = gpu.render_image_host(other, SEED, n_devices=n_dev)
                builds, updates = shim.rt_hip_cache_builds() - b0, shim.rt_hip_cache_updates() - u0
                in_place = mat_on and (move_on or not moves)
                assert (builds, updates) == ((1, 1) if in_place else (2, 0)), \
                    f"{what}, material updates {mat_on}, scene updates {move_on}, {n_dev} devices: {builds} builds, {updates} updates"
                for frame_ in (got, again):
                    assert np.array_equal(want[0].view(np.uint32), frame_[0].view(np.uint32)) and np.array_equal(want[1], frame_[1]), what
                    assert want[2] == frame_[2], what
    host.rt_set_material_updates(0)
    host.rt_set_scene_updates(0)
    shim.rt_hip_set_device_map(None, 0)
    shim.rt_hip_release_cache()
    for s in (base, recoloured, moved_too):
        s.free()


def test_cached_context_sizes_its_chunk_workspace_for_the_new_flag_class(gpu):
    """the cached context keeps one chunk workspace a device, sized by the scene's flag class: the plain record, or the six times
    larger windowed one of the M_REFRACTION forms.  A first frame at 256 spp is a CHUNKED launch (the workspace exists, at the plain
    size); then a ball turns to glass in place, and the next chunked launch takes a windowed kernel: it must find a workspace of
    the windowed size.  Then a checkered wall on top, and back to M0.  Every frame equals a fresh context's, on 1 and 2 logical
    devices."""
    from rt_amd import abi
    from rt_amd.dist import n_tiles
    shim, host = abi.load_shim(), abi.load_host()
    spp = 256
    base = SCENES["room"]()
    chain = {name: (c, e, f) for name, c, e, f, _ in steps(base)}
    c, e, f = chain["a sphere to glass"]
    glass = SCENES["room"]()
    E.set_materials(glass, c, e, f)
    both = SCENES["room"]()
    f2 = f.copy()
    f2[WALL] |= E.M_CHECKERED
    E.set_materials(both, c, e, f2)
    gs, gg = gpu.GpuScene(base), gpu.GpuScene(glass)
    total = n_tiles(base.width, base.height)
    for share in (total, total // 2):
        assert gs.suggest_chunks(share, spp) > 1 and gg.suggest_chunks(share, spp) > 1, "both frames must be chunked launches"
    assert gs.kernel_name() != gg.kernel_name() and gg.material_bounds()["any_refract"] and not gs.material_bounds()["any_refract"]
    assert shim.rt_hip_scene_chunk_workspace_bytes(gg.handle, total) > shim.rt_hip_scene_chunk_workspace_bytes(gs.handle, total)
    for s in (gs, gg):
        s.close()
    order = [base, glass, both, glass, base]
    for map_, n_dev in ((None, 1), ((C.c_int * 2)(0, 0), 2)):
        assert shim.rt_hip_set_device_map(map_, 2 if map_ is not None else 0) == 0
        host.rt_set_material_updates(0)
        want = []
        for sc in order[:3]:
            shim.rt_hip_release_cache()
            want.append(gpu.render_image_host(sc, SEED, n_devices=n_dev, samples=spp))       # a fresh context each
        want += [want[1], want[0]]
        assert not np.array_equal(want[0][0], want[1][0]) and not np.array_equal(want[1][0], want[2][0])
        host.rt_set_material_updates(1)
        shim.rt_hip_release_cache()
        b0, u0 = shim.rt_hip_cache_builds(), shim.rt_hip_cache_updates()
        for k, sc in enumerate(order):
            got = gpu.render_image_host(sc, SEED, n_devices=n_dev, samples=spp)
            what = f"frame {k}, {n_dev} devices"
            assert np.array_equal(want[k][0].view(np.uint32), got[0].view(np.uint32)) and np.array_equal(want[k][1], got[1]), what
            assert want[k][2] == got[2], what
        assert (shim.rt_hip_cache_builds() - b0, shim.rt_hip_cache_updates() - u0) == (1, 4)
    host.rt_set_material_updates(0)
    shim.rt_hip_set_device_map(None, 0)
    shim.rt_hip_release_cache()
    for s in (base, glass, both):
        s.free()


def test_host_library_runs_a_round_on_a_changed_emission(gpu):
    """rt_set_probe_update with rt_set_material_updates(1): the second frame is update_materials_host, one round on the kept state
    and the preview; with the switch off it is the full bake of the new scene"""
    import torch
    import probe_expected as P
    from rt_amd import abi, scene as Sc
    from test_gpu_probe_update_host import COUNT, DEPTH, H, HYST, LIGHT, RAYS, SAMPLES, W, Library, _full_frame, _grid_over_the_scene, _host

    def dim(sc):
        em = sc.objects[LIGHT].emission
        assert max(em.tuple()) > 0
        sc.objects[LIGHT].emission = abi.Vec3(em.x * 0.25, em.y * 0.5, em.z * 0.125)

    frames = {}
    for on in (1, 0):
        sc = Sc.build_scene(4, W, H, 1, DEPTH)
        with Library(0) as lib:
            lib.host.rt_set_material_updates(on)
            lib.host.rt_set_probe_update(RAYS, HYST)
            try:
                first = lib.render(sc)
                dim(sc)
                frames[on] = (first, lib.render(sc))
            finally:
                lib.host.rt_set_material_updates(0)
        if not on:
            want8, want, _ = _full_frame(gpu, sc, 0)
            assert frames[0][1][0].tobytes() == want8.tobytes() and frames[0][1][1].tobytes() == want.tobytes(), "off: the full bake"
        sc.free()
    assert frames[1][0][1].tobytes() == frames[0][0][1].tobytes(), "the first frame is the full bake either way"
    assert frames[1][1][1].tobytes() != frames[0][1][1].tobytes(), "a round on the kept state is not the full bake"
    # the composition
    sc2 = Sc.build_scene(4, W, H, 1, DEPTH)
    gs = gpu.GpuScene(sc2)
    try:
        grid, _ = _grid_over_the_scene(gs)
        coeff = gs.bake_probe_grid(grid, SAMPLES, P.SEED, max_depth=DEPTH).clone()
        age = torch.ones(COUNT[0] * COUNT[1] * COUNT[2], dtype=torch.int32, device=gs.dev)
        for u in (0, 1):
            if u:
                dim(sc2)
                c, e, f = E.materials_of(sc2)
                gs.update_materials(c, e, f)
                gs.probe_grid_update(grid, abi.probe_update(round=u, hysteresis=HYST), RAYS, P.SEED, coeff, age, None, None, max_depth=DEPTH)
            rgb, rgb8 = gs.probe_preview(grid, coeff, aov_samples=1, seed=P.SEED)
            fb, lin = frames[1][u]
            assert (fb == _host(rgb8)).all() and (lin.view(np.uint32) == _host(rgb).view(np.uint32)).all(), f"frame {u}"
        assert (_host(age) == 2).all()
    finally:
        gs.close()
        sc2.free()

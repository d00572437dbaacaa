"""Moving spheres: GpuScene.update_spheres (rt_hip_scene_update_spheres, raytracer.c_amd/csrc/scene_update.hip: k_update_spheres).

The contract: after an update the records (read_spheres), the scalars a scene derives from its spheres (sphere_bounds, the reach),
kernel_name, and the frames, bytes and counters of every launch equal, bit for bit, a scene freshly created from the same spheres.
  1. per scene class -- the smallest shapes at which a path can go wrong (SCENES) -- and per move: (a) identity, (b) a seeded jitter
     of every small sphere, (c) everything translated by 40 (reach, near_R and the tables change), (d) leading wall 3 shrunk to
     radius 500 (n_big 6 -> 2: the room has six leading walls, its two lights are small; the reach grows), (e) a wall's centre sent to 2e17 and brought back (wide_range flips, the kernel
     changes and returns): state and frame equal the fresh scene's, and the frame meets the oracle through util.assert_parity;
  2. ray queries (also against the compiled reference), radiance queries, pixel queries and first-hit buffers after (b);
  3. ten updates in a row: update_info counts 10, the pools do not grow;
  4. a vertex update and a sphere update interleaved on the tris=400 scene;
  5. every refusal leaves records and frame as they were;
  6. the device form fed from a torch tensor and the host form give the same bytes;
  7. the C host under rt_set_scene_updates(1) at 1 and 2 logical devices: one build and one update for a sphere-only move and for
     a sphere-and-vertex move, two builds with the switch off, frames equal to a fresh context's;
  8. the PT_DIAG re-check of the skipping rules after (b) and (d) (tests/sphere_update_diag_child.py): 0 violations.
(e) moves a WALL: a small sphere 2e17 out would be part of the reach, and a launch refuses near_R >= 1e15.
"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import scene_update_meshes as U
import sphere_update_expected as E
from conftest import SEED
from test_gpu_scene_update import assert_same_frame, frame, move_scene as move_vertices, same_bits_or_nan, tris_of
from util import assert_parity, class_scene, fixed_point_floor

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = {
    "packed4": dict(n_packed=4),                 # staged, sign form, the leading walls pruned
    "packed31": dict(n_packed=31), "packed32": dict(n_packed=32), "packed33": dict(n_packed=33),   # the fp16 matrix filter's 32
    "packed80": dict(n_packed=80),               # streamed by preference
    "packed300": dict(n_packed=300),             # too large to stage
    "refr": dict(n_packed=4, refr=True),         # the pending-ray pool
    "chk": dict(n_packed=4, chk=True),
    "wide": dict(n_packed=4, wide=True),
    "tris12": dict(n_packed=4, tris=12),         # the flat _tri form
    "tris400_round": dict(n_packed=4, tris=400, round_mesh=True),   # the parked walk that filters the spheres alone
}
FAR_WALL = 5
ELIMIT = -5      # RT_HIP_ELIMIT (include/rt_hip.h)


@pytest.fixture(scope="module")
def gpu():
    import torch
    from rt_amd import abi, gpu as G
    assert abi.load_shim().rt_hip_device_count() >= 1, "no HIP device: the GPU tests must run on the GPU box"
    assert torch.cuda.is_available()
    yield G
    abi.load_host().rt_set_scene_updates(0)
    abi.load_shim().rt_hip_set_device_map(None, 0)


def state(gs):
    s = gs.read_spheres()
    s.update(sphere_bounds=gs.sphere_bounds(), reach=gs.bounds()["reach"], kernel=gs.kernel_name(), whitted=gs.kernel_name("whitted"))
    return s


def assert_same_state(got, want, what):
    for f in ("entry", "geom4"):
        assert same_bits_or_nan(got[f], want[f]), f"{what}: {f} differs from the fresh scene's"
    gb, wb = got["sphere_bounds"], want["sphere_bounds"]
    for f in ("reach_spheres", "max_center"):
        assert np.float64(gb[f]).view(np.uint64) == np.float64(wb[f]).view(np.uint64), f"{what}: {f} {gb[f]!r} != {wb[f]!r}"
    for f in ("wide_range", "n_big"):
        assert gb[f] == wb[f], f"{what}: {f} {gb[f]} != {wb[f]}"
    for f in ("big_r", "big_c"):
        assert E.same_bits(gb[f], wb[f]), f"{what}: {f} {gb[f]} != {wb[f]}"
    assert np.float64(got["reach"]).view(np.uint64) == np.float64(want["reach"]).view(np.uint64), f"{what}: reach {got['reach']!r} != {want['reach']!r}"
    for f in ("kernel", "whitted"):
        assert got[f] == want[f], f"{what}: {f} {got[f]} != {want[f]}"


def as_input(spheres, k):
    """the new spheres as a device tensor (even k: the device entry) or a numpy array (odd k: the host entry)"""
    import torch
    return torch.tensor(spheres, dtype=torch.float64, device="cuda") if k % 2 == 0 else np.ascontiguousarray(spheres)


def moved_scene(cls, spheres, **size):
    sc = class_scene(**dict(cls, **size))
    E.move_scene(sc, spheres)
    return sc


@pytest.mark.parametrize("name", list(SCENES))
def test_update_equals_a_fresh_scene(gpu, pt, name):
    cls = SCENES[name]
    base = class_scene(**cls)
    s0 = E.spheres_of(base)
    gs = gpu.GpuScene(base)
    before, st0 = frame(gs), state(gs)
    assert E.same_bits(st0["entry"], E.expected(s0)["entry"]), f"{name}: a created scene's records against the numpy restatement"
    if not cls.get("wide"):
        assert st0["sphere_bounds"]["n_big"] == 6 and not st0["sphere_bounds"]["wide_range"]
    steps = [("identity", E.MOVES["identity"](s0)), ("jitter", E.jitter(s0)), ("translate", E.translated(s0)),
             ("wall_shrunk", E.wall_shrunk(s0)), ("far", E.far_centre(s0, FAR_WALL)), ("back", s0.copy())]
    for k, (step, new) in enumerate(steps):
        what = f"{name} {step}"
        gs.update_spheres(as_input(new, k))
        moved = moved_scene(cls, new)
        fresh = gpu.GpuScene(moved)
        got_state, want_state = state(gs), state(fresh)
        assert_same_state(got_state, want_state, what)
        want = E.expected(new)
        assert E.same_bits(got_state["entry"], want["entry"]) and E.same_bits(got_state["geom4"], want["geom4"]), f"{what}: numpy's records"
        b = got_state["sphere_bounds"]
        assert (b["n_big"], b["reach_spheres"], b["max_center"]) == (want["n_big"], want["reach_spheres"], want["max_center"]), what
        got, exp = frame(gs), frame(fresh)
        assert_same_frame(got, exp, what)
        mean, rgb8, ost = pt.render_pixels(moved, SEED)
        assert_parity(got[0], got[1], got[2], mean, rgb8, ost, what=what, hdr=True, abs_floor=fixed_point_floor(moved))
        if step in ("identity", "back"):
            assert_same_frame(got, before, what + " against the frame before any update")
            assert_same_state(got_state, st0, what + " against the state before any update")
        if step == "translate":
            assert got_state["reach"] > st0["reach"] + 10
        if step == "wall_shrunk" and not cls.get("wide"):
            assert b["n_big"] == 2 and got_state["reach"] > 1000 > st0["reach"]
        if step == "far" and not cls.get("wide"):
            assert b["wide_range"] and got_state["kernel"] != st0["kernel"] and got[3] != before[3], f"{what}: {got_state['kernel']}"
        fresh.close()
        moved.free()
    assert gs.update_info()["updates"] == len(steps)
    gs.close()
    base.free()


def _np(out):
    import torch
    torch.cuda.synchronize()
    res = {f: t.cpu().numpy() for f, t in out.items()}
    return {f: np.ascontiguousarray(x).view(np.uint8) for f, x in res.items()}


def test_queries_and_first_hit_buffers_after_an_update(gpu, ref_mesh):
    import query_expected as Q
    import refine_expected as R
    cls = SCENES["packed33"]
    base = class_scene(**cls)
    new = E.jitter(E.spheres_of(base))
    moved = moved_scene(cls, new)
    rays = Q.ray_set(moved)
    exp = Q.expected(ref_mesh(5), moved, rays=rays)
    pixels = R.pixel_list(moved.width, moved.height)
    gs, fresh = gpu.GpuScene(base), gpu.GpuScene(moved)
    gs.update_spheres(as_input(new, 0))
    got = {f: t.cpu().numpy() for f, t in gs.query_rays(rays).items()}
    msg = Q.mismatch(got, exp)
    assert not msg, msg
    assert (got["status"].view(np.uint32) == 1).sum() > 20, "the rays must meet spheres"
    calls = {"query_rays": lambda s: _np(s.query_rays(rays)),
             "trace_rays": lambda s: _np(s.trace_rays(rays[:65], 2, SEED, want=("status", "radiance", "samples", "paths", "casts"))),
             "trace_pixels": lambda s: _np(s.trace_pixels(pixels, 2, SEED, want=("status", "radiance", "samples", "paths", "casts"))),
             "render_aov": lambda s: {f: np.ascontiguousarray(x).view(np.uint8) for f, x in s.aov_image(SEED, 2).items()}}
    for form, call in calls.items():
        a, e = call(gs), call(fresh)
        assert a.keys() == e.keys()
        for f in a:
            assert np.array_equal(a[f], e[f]), f"{form}: {f} differs from the fresh scene's"
        assert gs.launch_status() == 0
    for s in (gs, fresh):
        s.close()
    for s in (base, moved):
        s.free()


def test_ten_updates_in_a_row(gpu, pt):
    from rt_amd import abi
    shim = abi.load_shim()
    cls = SCENES["refr"]
    base = class_scene(**cls)
    s0 = E.spheres_of(base)
    gs = gpu.GpuScene(base)
    frame(gs)

    def pools():
        park, pend = C.c_size_t(0), C.c_size_t(0)
        assert shim.rt_hip_pool_bytes(0, C.byref(park), C.byref(pend)) == 0
        return park.value, pend.value

    pools0 = pools()
    for k in range(10):
        new = E.jitter(s0, seed=100 + k)
        gs.update_spheres(as_input(new, k))
        got = frame(gs)
        if k in (0, 9):
            moved = moved_scene(cls, new)
            mean, rgb8, ost = pt.render_pixels(moved, SEED)
            assert_parity(got[0], got[1], got[2], mean, rgb8, ost, what=f"jitter {k}", hdr=True, abs_floor=fixed_point_floor(moved))
            moved.free()
    assert gs.update_info()["updates"] == 10 and gs.update_info()["last_seconds"] > 0
    assert pools() == pools0, "an update must not grow the device's pools"
    gs.close()
    base.free()


def test_vertex_and_sphere_updates_interleaved(gpu, pt):
    cls = SCENES["tris400_round"]
    base = class_scene(**cls)
    s0, t0 = E.spheres_of(base), tris_of(base)
    gs = gpu.GpuScene(base, bvh="device")
    frame(gs)
    s1, t1, s2 = E.jitter(s0), U.scale_wobble(t0), E.translated(E.jitter(s0, seed=12), by=3.0)
    for k, (spheres, tris, what) in enumerate(((s1, None, "spheres"), (None, t1, "then vertices"), (s2, None, "then spheres again"))):
        if spheres is not None:
            gs.update_spheres(as_input(spheres, k))
        else:
            gs.update_vertices(np.ascontiguousarray(tris))
        moved = moved_scene(cls, s1 if k < 2 else s2)
        if k:
            move_vertices(moved, t1)
        fresh = gpu.GpuScene(moved, bvh="device")
        assert_same_state(state(gs), state(fresh), what)
        assert gs.bounds() == fresh.bounds(), what
        got = frame(gs)
        assert_same_frame(got, frame(fresh), what)
        mean, rgb8, ost = pt.render_pixels(moved, SEED)
        assert_parity(got[0], got[1], got[2], mean, rgb8, ost, what=what, hdr=True, abs_floor=fixed_point_floor(moved))
        fresh.close()
        moved.free()
    assert gs.update_info()["updates"] == 3
    gs.close()
    base.free()


def max_vertex(tris):
    """max |vertex| as the shim forms it: sqrt((x x + y y) + z z)"""
    v = np.asarray(tris, dtype=np.float64).reshape(-1, 3)
    return float(np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]).max())


@pytest.mark.parametrize("order", ["vertices_first", "spheres_first"])
def test_interleaved_updates_where_the_mesh_sets_the_reach(gpu, pt, order):
    """the reach is the larger of the spheres' part and the vertices' part, and each update must join its own NEW part with the
    other's CURRENT one: the mesh scaled by 6 about the origin reaches past every small sphere (first pair of updates: the
    vertices' part grows), then comes back (second pair: it shrinks), in both orders of the pair"""
    cls = SCENES["tris400_round"]
    base = class_scene(**cls)
    s0, t0 = E.spheres_of(base), tris_of(base)
    far = t0 * 6.0
    gs = gpu.GpuScene(base, bvh="device")
    reach0 = state(gs)["sphere_bounds"]["reach_spheres"]
    assert max_vertex(t0) < reach0 < max_vertex(far) - 10, "the mesh must set the reach when it is far, the spheres when it is near"
    frame(gs)
    for k, (spheres, tris) in enumerate(((E.jitter(s0), far), (E.jitter(s0, seed=12), t0))):
        calls = [lambda: gs.update_vertices(as_input(tris, k)), lambda: gs.update_spheres(as_input(spheres, k + 1))]
        for call in (calls if order == "vertices_first" else calls[::-1]):
            call()
        what = f"{order}, pair {k}"
        moved = moved_scene(cls, spheres)
        move_vertices(moved, tris)
        fresh = gpu.GpuScene(moved, bvh="device")
        assert gs.bounds() == fresh.bounds(), f"{what}: {gs.bounds()} != {fresh.bounds()}"
        assert_same_state(state(gs), state(fresh), what)
        want_reach = max(max_vertex(tris), E.expected(spheres)["reach_spheres"])
        assert gs.bounds()["reach"] == want_reach, f"{what}: reach {gs.bounds()['reach']!r}, numpy {want_reach!r}"
        got = frame(gs)
        assert_same_frame(got, frame(fresh), what)
        mean, rgb8, ost = pt.render_pixels(moved, SEED)
        assert_parity(got[0], got[1], got[2], mean, rgb8, ost, what=what, hdr=True, abs_floor=fixed_point_floor(moved))
        fresh.close()
        moved.free()
    assert gs.update_info()["updates"] == 4
    gs.close()
    base.free()


def test_refusals_leave_the_scene_alone(gpu):
    import torch
    from rt_amd import abi
    shim = abi.load_shim()
    cls = SCENES["packed33"]
    base = class_scene(**cls)
    s0 = E.spheres_of(base)
    n = len(s0)
    gs = gpu.GpuScene(base)
    st0, f0 = state(gs), frame(gs)
    new = E.jitter(s0)

    def refused(call, word, code=abi.EINVAL):
        with pytest.raises(gpu.ShimError) as e:
            call()
        assert f"({code})" in str(e.value) and word in str(e.value), str(e.value)
        assert_same_state(state(gs), st0, word)
        assert_same_frame(frame(gs), f0, word)
        assert gs.update_info()["updates"] == 0

    refused(lambda: gpu._check(shim.rt_hip_scene_update_spheres_host(gs.handle, new.ctypes.data, n - 1), "update"), "count")
    refused(lambda: gpu._check(shim.rt_hip_scene_update_spheres_host(gs.handle, None, n), "update"), "required")
    refused(lambda: gpu._check(shim.rt_hip_scene_update_spheres(gs.handle, None, n), "update"), "required")
    refused(lambda: gs.update_spheres(torch.tensor(new)), "device memory")            # a host tensor at the device entry
    acc = gs.accumulate(SEED, 4)
    refused(lambda: gs.update_spheres(new), "accumulation")
    acc.close()
    for bad_r in (1e-101, 1e101, np.nan, 0.0, -1e101):                                # rt_hip_scene_create's rule, from either entry
        bad = new.copy()
        bad[n - 2, 3] = bad_r
        refused(lambda: gs.update_spheres(bad), "radius", ELIMIT)
        refused(lambda: gs.update_spheres(torch.tensor(bad, device="cuda")), "radius", ELIMIT)
    # a centre rt_hip_scene_create accepts is accepted: -0.0, and once nothing stands in the way the same spheres go through
    new[n - 1, 0] = -0.0
    gs.update_spheres(new)
    moved = moved_scene(cls, new)
    fresh = gpu.GpuScene(moved)
    assert_same_state(state(gs), state(fresh), "after the refusals")
    assert_same_frame(frame(gs), frame(fresh), "after the refusals")
    assert gs.update_info()["updates"] == 1
    for s in (gs, fresh):
        s.close()
    for s in (base, moved):
        s.free()


def test_a_scene_without_spheres_is_refused(gpu):
    """the refusal that needs a scene of its own: a mesh-only scene, whatever the count.  (Two refusals are not reached from here:
    no call gives out an address inside a scene's allocation, and a launch "being submitted" needs a second thread inside the
    shim.)"""
    import torch
    from rt_amd import abi, scene as S
    shim = abi.load_shim()
    tris = np.array([[[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]])
    sc = S.custom_scene([], 48, 32, 3, 5, (0, 0, 4), (0, 0, 0), meshes=[dict(flags=abi.M_DEFAULT, color=(0.8, 0.7, 0.6), triangles=tris)])
    gs = gpu.GpuScene(sc)
    st0, tri0, f0 = state(gs), gs.read_triangles(), frame(gs)
    buf = torch.zeros((1, 4), dtype=torch.float64, device="cuda")
    host_buf = np.ones((1, 4))
    for rc in (shim.rt_hip_scene_update_spheres(gs.handle, C.c_void_p(buf.data_ptr()), 0),
               shim.rt_hip_scene_update_spheres(gs.handle, C.c_void_p(buf.data_ptr()), 1),
               shim.rt_hip_scene_update_spheres_host(gs.handle, host_buf.ctypes.data, 1)):
        assert rc == abi.EINVAL and b"no spheres" in shim.rt_hip_last_error()
        assert_same_state(state(gs), st0, "no spheres")
        assert all(same_bits_or_nan(a, b) for a, b in zip(gs.read_triangles().values(), tri0.values()))
        assert_same_frame(frame(gs), f0, "no spheres")
    assert gs.update_info()["updates"] == 0
    gs.close()


def test_device_and_host_forms_give_the_same_bytes(gpu):
    import torch
    cls = SCENES["packed80"]
    base = class_scene(**cls)
    new = E.translated(E.jitter(E.spheres_of(base)), by=-7.0)
    a, b = gpu.GpuScene(base), gpu.GpuScene(base)
    t = torch.tensor(new, dtype=torch.float64, device="cuda")
    a.update_spheres(t * 1.0)                      # a tensor another kernel has just written on torch's stream
    b.update_spheres(new)
    assert_same_state(state(a), state(b), "device form against host form")
    assert_same_frame(frame(a), frame(b), "device form against host form")
    assert torch.equal(a.spheres(), t) and torch.equal(b.spheres(), t), "spheres(): the current ones"
    for s in (a, b):
        s.close()
    base.free()


def test_c_host_updates_the_cached_scene(gpu):
    """rt_hip_render_image under rt_set_scene_updates: moved spheres -- alone, or with moved vertices -- update the cached context
    in place (one build, one update), also on 2 logical devices; with the default 0 the second call rebuilds"""
    from rt_amd import abi
    shim, host = abi.load_shim(), abi.load_host()
    cls = dict(n_packed=4, tris=400, round_mesh=True)
    base = class_scene(**cls)
    s1 = E.jitter(E.spheres_of(base))
    only_spheres = moved_scene(cls, s1)
    both = moved_scene(cls, s1)
    move_vertices(both, U.scale_wobble(tris_of(base)))
    # ... and with the mesh scaled past every small sphere: the vertices' part of the reach changes and decides it
    both_far = moved_scene(cls, s1)
    move_vertices(both_far, tris_of(base) * 6.0)
    assert max_vertex(tris_of(both_far)) - 10 > E.expected(s1)["reach_spheres"] > max_vertex(tris_of(base))
    for map_, n_dev in ((None, 1), ((C.c_int * 2)(0, 0), 2)):
        assert shim.rt_hip_set_device_map(map_, 2 if map_ is not None else 0) == 0
        for moved, what in ((only_spheres, "spheres"), (both, "spheres and vertices"), (both_far, "spheres and far vertices")):
            host.rt_set_scene_updates(0)
            shim.rt_hip_release_cache()
            want = gpu.render_image_host(moved, SEED, n_devices=n_dev)          # a fresh context for the moved scene
            for on in (1, 0):
                host.rt_set_scene_updates(on)
                shim.rt_hip_release_cache()
                b0, u0 = shim.rt_hip_cache_builds(), shim.rt_hip_cache_updates()
                gpu.render_image_host(base, SEED, n_devices=n_dev)
                got = gpu.render_image_host(moved, SEED, n_devices=n_dev)
                again = gpu.render_image_host(moved, SEED, n_devices=n_dev)
                builds, updates = shim.rt_hip_cache_builds() - b0, shim.rt_hip_cache_updates() - u0
                assert (builds, updates) == ((1, 1) if on else (2, 0)), f"{what}, updates {on}, {n_dev} devices: {builds} builds, {updates} updates"
                for other in (got, again):
                    assert np.array_equal(want[0].view(np.uint32), other[0].view(np.uint32)) and np.array_equal(want[1], other[1]), what
                    assert want[2] == other[2], what
    # a changed colour is no move: the context is rebuilt, updates or not
    host.rt_set_scene_updates(1)
    shim.rt_hip_release_cache()
    b0, u0 = shim.rt_hip_cache_builds(), shim.rt_hip_cache_updates()
    gpu.render_image_host(base, SEED, n_devices=1)
    from rt_amd import abi as A
    only_spheres.objects[9].color = A.Vec3(0.5, 0.5, 0.5)
    gpu.render_image_host(only_spheres, SEED, n_devices=1)
    assert (shim.rt_hip_cache_builds() - b0, shim.rt_hip_cache_updates() - u0) == (2, 0)
    host.rt_set_scene_updates(0)
    shim.rt_hip_set_device_map(None, 0)
    shim.rt_hip_release_cache()
    for s in (base, only_spheres, both, both_far):
        s.free()


def test_skipping_rules_hold_on_updated_scenes():
    """the n_packed=33 and n_packed=4 scenes after moves (b) and (d), in place, through the PT_DIAG build: the exhaustive re-checks
    of the conservative rules (filter, matrix filter, wall pruning) find nothing"""
    env = dict(os.environ, RT_HIP_SHIM_PATH=os.path.join(ROOT, "raytracer.c_amd", "csrc", "librt_hip_diag.so"))
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "sphere_update_diag_child.py")], env=env, capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    recs = [json.loads(l) for l in out.stdout.strip().splitlines() if l.startswith("{")]
    print(recs)
    assert len(recs) == 4
    for rec in recs:
        assert rec["violations"] == 0, rec
        assert rec["casts"] > 0 and rec["filter_evals"] > 0, f"the check was vacuous: {rec}"

"""One scene through every way of changing it, in a row, with two table sets alive: the shim's shared guard (SceneWrite), its
shared drain of the table sets and its shared install of a device-built tree all act on the same live sets only here.

The scene: the n257 shell x 3 and four small spheres, device builder, 48 x 32 at 4 samples.  It is rendered from its own camera
and from twice as far (another near_R: a second, owned table set), then takes a vertex update, a sphere update, a rebuild and a
vertex update again.  After each step the read-backs (triangle records, bounds, hull facets, sphere records and scalars, kernel
names; after the rebuild also nodes, order and bvh_info) and the frame at both distances equal, bit for bit, those of a scene
freshly created from the same data with the device builder, and rt_hip_pool_bytes is what it was."""
import ctypes as C

import numpy as np
import pytest

import bvh_sweep_meshes as M
import scene_update_meshes as U
import sphere_update_expected as E
from conftest import SEED
from test_gpu_bvh_rebuild import assert_same_tree, far_camera
from test_gpu_scene_update import assert_same_frame, assert_same_state, frame, state
from test_gpu_sphere_update import assert_same_state as assert_same_spheres, state as sphere_state

pytestmark = pytest.mark.gpu
W, H = 48, 32


@pytest.fixture(scope="module")
def gpu():
    import torch
    from rt_amd import abi, gpu as G
    assert abi.load_shim().rt_hip_device_count() >= 1, "no HIP device: the GPU tests must run on the GPU box"
    assert torch.cuda.is_available()
    return G


def scene_of(tris, spheres):
    from rt_amd import abi, scene as S
    objs = [dict(flags=abi.M_DEFAULT, radius=float(s[3]), center=tuple(map(float, s[:3])), color=(0.9, 0.8 - 0.2 * i, 0.3 + 0.2 * i),
                 emission=(8, 8, 8) if i == 0 else (0, 0, 0)) for i, s in enumerate(spheres)]
    return S.custom_scene(objs, W, H, 4, 8, (0, 0, 4), (0, 0, 0),
                          meshes=[dict(flags=abi.M_DEFAULT, color=(0.8, 0.7, 0.6), triangles=np.asarray(tris, dtype=np.float64))])


def far_frame(gs, cam):
    import torch
    t, t8, st = gs.render_tiles(SEED, 0, 1, ((W + 7) // 8) * ((H + 7) // 8), camera=cam)
    torch.cuda.synchronize()
    assert gs.launch_status() == 0
    return t.cpu().numpy().view(np.uint32), t8.cpu().numpy(), st.cpu().numpy()


def pools():
    from rt_amd import abi
    park, pend = C.c_size_t(0), C.c_size_t(0)
    assert abi.load_shim().rt_hip_pool_bytes(0, C.byref(park), C.byref(pend)) == 0
    return park.value, pend.value


def test_every_mutation_in_a_row_on_live_table_sets(gpu):
    import torch
    t0 = np.array(M.mesh("n257")) * 3.0
    s0 = np.array([[0.0, 18.0, 0.0, 4.0], [2.5, 0.5, -1.0, 0.75], [-2.0, -1.5, 0.5, 0.5], [0.5, 2.0, 1.5, 0.25]])
    s1 = s0 + np.array([[0.5, -1.0, 0.25, 0.5], [-0.75, 0.25, 0.5, -0.25], [0.25, 0.5, -0.5, 0.125], [-1.0, -0.5, 0.25, 0.25]])
    t1, t2 = U.scale_wobble(t0), U.mirror(t0)
    base = scene_of(t0, s0)
    cam = far_camera(base)
    gs = gpu.GpuScene(base, bvh="device")
    frame(gs)
    far_frame(gs, cam)                                  # two table sets are alive from here on
    pools0 = pools()
    steps = [("vertex update", lambda: gs.update_vertices(torch.tensor(t1, dtype=torch.float64, device="cuda")), t1, s0),
             ("sphere update", lambda: gs.update_spheres(np.ascontiguousarray(s1)), t1, s1),
             ("rebuild", gs.rebuild_bvh, t1, s1),
             ("vertex update again", lambda: gs.update_vertices(np.ascontiguousarray(t2)), t2, s1)]
    for what, change, tris, spheres in steps:
        change()
        moved = scene_of(tris, spheres)
        fresh = gpu.GpuScene(moved, bvh="device")
        assert_same_state(state(gs), state(fresh), what)
        assert_same_spheres(sphere_state(gs), sphere_state(fresh), what)
        assert E.same_bits(sphere_state(gs)["entry"], E.expected(spheres)["entry"]), f"{what}: the sphere records against numpy's"
        if what == "rebuild":
            assert_same_tree(gs, fresh, what)
        assert_same_frame(frame(gs), frame(fresh), what)
        for x, y in zip(far_frame(gs, cam), far_frame(fresh, cam)):
            assert np.array_equal(x, y), f"{what}: the far camera's frame differs from the fresh scene's"
        fresh.close()
        moved.free()
        assert pools() == pools0, f"{what}: the pools went from {pools0} to {pools()}"
    assert gs.update_info()["updates"] == 3 and gs.rebuild_info()["rebuilds"] == 1
    gs.close()
    base.free()

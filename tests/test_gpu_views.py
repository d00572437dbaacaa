"""Every row of the kernel pick table under other cameras, and with its scene far out or scaled (util.VARIANTS).

The rules that let a kernel skip an exact fp64 test depend on what the rows' one camera fixes: the tile cones of tile_cull
(pt_filter.h: corner vectors, 1e-5 margins, the cos_t <= 0 branch of cones wider than 90 degrees) and the margins that widen
by e A with A = |c| + near_R (the packed-fp32 filter, tri_may_hit32, mesh_bound_for, big_prune_for, hull_margin_for).  Here
each row renders at 48 x 32 through inside, steep, telephoto, wide, sheared and near_plane cameras, and with the whole
scene moved 2e7 out or scaled by 1e-3 and 1e3; pixels, bytes and counters must be the oracle's (the variants are pinned
against the compiled reference, and shown to reach their edges, by tests/test_views_cpu.py).  Then three smaller cases: an
accumulation whose table sets are recycled between its passes, the C host's cached context under a moving camera, and a
hand-built camera on logical devices.
"""
import ctypes as C

import numpy as np
import pytest

from conftest import SEED
from test_gpu_parity import PICK_ROWS, _WP
from test_views_cpu import ROW_IDS
from util import VARIANTS, assert_parity, class_scene, fixed_point_floor, pick_moves, view_variant

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch
    from rt_amd import abi, gpu as G
    assert abi.load_shim().rt_hip_device_count() >= 1, "no HIP device: the GPU tests must run on the GPU box"
    assert torch.cuda.is_available()
    yield G
    abi.load_shim().rt_hip_set_device_map(None, 0)


@pytest.mark.parametrize("cls,integrator,faults,kernel", PICK_ROWS, ids=ROW_IDS)
def test_every_row_renders_the_oracle_s_frame_under_every_view(gpu, pt, cls, integrator, faults, kernel):
    from rt_amd import abi
    shim = abi.load_shim()
    base = class_scene(**cls)
    done = []
    for variant in VARIANTS:
        if pick_moves(cls, kernel, variant):   # the variant changes the scene's class (test_views_cpu.py: PICK_MOVES)
            continue
        sc = view_variant(base, variant)
        what = f"{kernel} {variant}"
        if faults & _WP:
            shim.rt_hip_release_cache()      # no pending-ray pool yet: the launch has to ask for the wide one
        shim.rt_hip_selftest_fail_alloc(faults)
        try:
            gs = gpu.GpuScene(sc)
            img, img8, st = gs.render_image(SEED, integrator=integrator)
            assert gs.last_launch_kernel() == kernel, f"{what}: took {gs.last_launch_kernel()}"
        finally:
            shim.rt_hip_selftest_fail_alloc(0)
        mean, rgb8, ost = pt.render_pixels(sc, SEED, integrator=integrator)
        assert_parity(img.cpu().numpy(), img8.cpu().numpy(), st, mean, rgb8, ost, what=what, hdr=True,
                      abs_floor=fixed_point_floor(sc))
        gs.close()
        done.append(variant)
    assert len(done) == len(VARIANTS) - (1 if cls.get("wide") else 0), done
    base.free()


def _camera_at(sc, dist):
    """init_camera on the rows' axis, `dist` from the origin: another near_R, so another table set"""
    from rt_amd import scene as S
    return S.make_camera(sc.width, sc.height, (0.0, 0.0, float(dist)), (0.0, 0.0, 0.0))


@pytest.mark.parametrize("cls,kernel", [(dict(n_packed=4, refr=True), "pt_render_tiles_refr_pool"),
                                        (dict(n_packed=4, tris=400), "pt_render_tiles_tri_queued"),
                                        (dict(n_packed=120), "pt_render_tiles_pool_mem_s")], ids=lambda x: x if isinstance(x, str) else "")
def test_accumulation_survives_table_sets_recycled_between_its_passes(gpu, cls, kernel):
    """an accumulation acquires its camera's table set (rt_hip_shim.hip: acquire_tables, RT_TABLE_SETS = 8 per scene) again
    for every pass; launches of the same scene at ten other camera distances between the passes recycle every set"""
    import torch
    sc = class_scene(**dict(cls, samples=4))
    gs = gpu.GpuScene(sc)
    total = gpu.n_tiles(sc.width, sc.height)
    t, t8, st = gs.render_tiles(SEED, 0, 1, total, chunks=gs.suggest_chunks(total))
    torch.cuda.synchronize()
    assert gs.last_launch_kernel() == kernel
    t, t8, st = t.clone(), t8.clone(), st.clone()
    acc = gs.accumulate(SEED, 4)
    stats = torch.zeros(4, dtype=torch.int64, device="cuda")
    for k, n in enumerate([1, 2, 1]):
        acc.add(n, stats)
        for j in range(10):   # 10 distances > RT_TABLE_SETS
            gs.render_tiles(SEED, 0, 1, total, camera=_camera_at(sc, 30.0 + 2.5 * j + 0.25 * k))
    at, at8 = acc.resolve()
    torch.cuda.synchronize()
    gs.launch_status()
    assert acc.kernel == kernel and acc.samples == 4
    assert np.array_equal(at.cpu().numpy(), t.cpu().numpy()), kernel
    assert np.array_equal(at8.cpu().numpy(), t8.cpu().numpy()), kernel
    assert stats.tolist() == st.tolist()
    acc.close()
    gs.close()


def test_c_host_cached_context_with_a_moving_camera(gpu, pt):
    """rt_hip_render_image keeps its context while the scene's bytes are unchanged: a camera that moves between frames
    (there, back) is the launch's, not the context's -- each frame is the oracle's, and nothing is rebuilt"""
    from rt_amd import abi
    shim = abi.load_shim()
    sc = class_scene(n_packed=4, tris=400, round_mesh=True)
    cams = [_camera_at(sc, 50.0), _camera_at(sc, 23.0), _camera_at(sc, 50.0)]
    sc.camera = cams[0]
    gpu.render_image_host(sc, SEED)
    b0 = shim.rt_hip_cache_builds()
    frames = []
    for cam in cams:
        sc.camera = cam
        img, img8, st, _ = gpu.render_image_host(sc, SEED)
        mean, rgb8, ost = pt.render_pixels(sc, SEED)
        assert_parity(img, img8, st, mean, rgb8, ost, what=f"camera at {cam.position.z}", hdr=True, abs_floor=fixed_point_floor(sc))
        frames.append((img, img8, st))
    assert shim.rt_hip_cache_builds() == b0, "a moving camera must not rebuild the context"
    assert np.array_equal(frames[0][0], frames[2][0]) and frames[0][2] == frames[2][2]
    assert not np.array_equal(frames[0][0], frames[1][0])


def test_logical_devices_with_a_hand_built_camera(gpu, pt):
    """one sheared, mirrored, off-centre frame on 3 logical devices (rt_hip_set_device_map): the one-device frame bit for bit"""
    from rt_amd import abi
    shim = abi.load_shim()
    sc = view_variant(class_scene(n_packed=4, tris=40), "sheared")
    assert shim.rt_hip_set_device_map(None, 0) == 0
    one = gpu.render_image_host(sc, SEED, n_devices=1)
    mean, rgb8, ost = pt.render_pixels(sc, SEED)
    assert_parity(one[0], one[1], one[2], mean, rgb8, ost, what="sheared G=1", hdr=True, abs_floor=fixed_point_floor(sc))
    arr = (C.c_int * 3)(0, 0, 0)
    assert shim.rt_hip_set_device_map(arr, 3) == 0, shim.rt_hip_last_error()
    try:
        three = gpu.render_image_host(sc, SEED, n_devices=3)
    finally:
        shim.rt_hip_set_device_map(None, 0)
    assert np.array_equal(three[0], one[0]) and np.array_equal(three[1], one[1]) and three[2] == one[2]

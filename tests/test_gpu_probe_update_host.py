"""rt_set_probe_update in the host library (include/raytracer.h), driven as tests/test_dropin.py drives it: with it on, render_ex() over a
moving sphere is a full bake, then one update round a call, each followed by the preview -- the composition of the public calls on
a scene that takes the same moves; with rays 0 the frame is the one without the call, byte for byte; a changed reach or resolution
falls back to the full bake."""
import ctypes as C

import numpy as np
import pytest

import probe_expected as P

pytestmark = pytest.mark.gpu

DEPTH = 4
W, H = 33, 17
COUNT, SAMPLES, RAYS, HYST = (4, 3, 4), 16, 8, 0.9
INNER, LIGHT = 6 + 27, 6 + 30   # config 4: a packed sphere well inside the room; the ceiling light, which sets the reach


@pytest.fixture
def gpu():
    import torch
    from rt_amd import abi, gpu as G
    assert abi.load_shim().rt_hip_device_count() >= 1, "no HIP device: the GPU tests must run on the GPU box"
    assert torch.cuda.is_available()
    return G


def _host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _grid_over_the_scene(gs):
    """rt_set_probe_grid's grid (include/raytracer.h): [-reach, reach] an axis about the world's origin -> (grid, reach)"""
    from rt_amd import abi
    reach = C.c_double()
    assert gs.shim.rt_hip_scene_bounds(gs.handle, None, None, C.byref(reach), None) == 0
    r = reach.value if reach.value > 0 else 1.0
    return abi.probe_grid([-r if n >= 2 else 0.0 for n in COUNT], [(2.0 * r) / float(n - 1) if n >= 2 else 1.0 for n in COUNT], COUNT), r


def _spheres(sc):
    return np.array([[o.center.x, o.center.y, o.center.z, o.radius] for o in sc.objects[:sc.n_objects]], dtype=np.float64).reshape(-1, 4)


def _move(sc, index, dx, dy, dz):
    c = sc.objects[index].center
    sc.objects[index].center = type(c)(c.x + dx, c.y + dy, c.z + dz)


class Library:
    """the host library with a probe grid, this test's seed and depth, and scene updates on; everything is put back on exit"""

    def __init__(self, res):
        from rt_amd import abi
        self.host, self.res = abi.load_host(), res

    def __enter__(self):
        h = self.host
        self.before = (h.rt_get_max_depth(), h.rt_get_seed())
        h.rt_set_max_depth(DEPTH)
        h.rt_set_seed(P.SEED)
        h.rt_set_probe_grid(*COUNT)
        h.rt_set_probe_visibility(self.res)
        h.rt_set_scene_updates(1)
        return self

    def __exit__(self, *exc):
        h = self.host
        h.rt_set_probe_update(0, HYST)
        h.rt_set_scene_updates(0)
        h.rt_set_probe_visibility(0)
        h.rt_set_probe_grid(0, 0, 0)
        h.rt_set_max_depth(self.before[0])
        h.rt_set_seed(self.before[1])

    def render(self, sc):
        from rt_amd import abi
        opt = abi.Options()
        opt.width, opt.height, opt.samples = W, H, SAMPLES
        fb, lin = np.zeros((H, W, 3), dtype=np.uint8), np.zeros((H, W, 3), dtype=np.float32)
        self.host.render_ex(fb.ctypes.data, lin.ctypes.data, sc.objects, sc.n_objects, None, 0, C.byref(sc.camera), C.byref(opt))
        return fb, lin


def _full_frame(gpu, sc, res):
    """today's frame of the scene as it stands: the host form that bakes and previews"""
    from rt_amd import abi
    gs = gpu.GpuScene(sc)
    grid, reach = _grid_over_the_scene(gs)
    gs.close()
    if res:
        lin, fb, _, _, _ = gpu.probe_preview_vis_host(sc, grid, abi.probe_vis(grid, res=res), SAMPLES, P.SEED, aov_samples=1, max_depth=DEPTH)
    else:
        lin, fb, _, _ = gpu.probe_preview_host(sc, grid, SAMPLES, P.SEED, aov_samples=1, max_depth=DEPTH)
    return fb, lin, reach


def test_setter():
    from rt_amd import abi
    host = abi.load_host()
    rays, h = C.c_int(-1), C.c_double(-1)
    host.rt_get_probe_update(C.byref(rays), C.byref(h))
    assert (rays.value, h.value) == (0, 0.9)   # off by default
    host.rt_set_probe_update(8, 0.5)
    host.rt_set_probe_update(4, 1.0)            # a hysteresis outside [0, 1) leaves it as it was
    host.rt_get_probe_update(C.byref(rays), C.byref(h))
    assert (rays.value, h.value) == (4, 0.5)
    host.rt_set_probe_update(-3, 0.9)
    host.rt_get_probe_update(C.byref(rays), None)
    assert rays.value == 0


@pytest.mark.parametrize("res", [4, 0])
def test_three_frames_are_a_bake_and_two_rounds(gpu, res):
    import torch
    from rt_amd import abi, scene as Sc
    sc = Sc.build_scene(4, W, H, 1, DEPTH)
    moves = [None, (1.0, 0.5, -0.75), (0.5, -0.25, 1.0)]
    with Library(res) as lib:
        lib.host.rt_set_probe_update(RAYS, HYST)
        got = []
        for mv in moves:
            if mv:
                _move(sc, INNER, *mv)
            got.append(lib.render(sc))
    # the composition, on a scene that takes the same moves in place
    sc2 = Sc.build_scene(4, W, H, 1, DEPTH)
    gs = gpu.GpuScene(sc2)
    try:
        grid, reach = _grid_over_the_scene(gs)
        vis = abi.probe_vis(grid, res=res) if res else None
        baked = gs.bake_probe_grid(grid, SAMPLES, P.SEED, max_depth=DEPTH, vis=vis)
        coeff, moments = (baked[0].clone(), baked[1].clone()) if res else (baked.clone(), None)
        age = torch.ones(COUNT[0] * COUNT[1] * COUNT[2], dtype=torch.int32, device=gs.dev)
        for u, mv in enumerate(moves):
            if mv:
                _move(sc2, INNER, *mv)
                gs.update_spheres(_spheres(sc2))
                again, reach2 = _grid_over_the_scene(gs)
                assert reach2 == reach, "the move must leave the reach as it is: this test is about the rounds"
                gs.probe_grid_update(grid, abi.probe_update(round=u, hysteresis=HYST), RAYS, P.SEED, coeff, age, vis, moments, max_depth=DEPTH)
            rgb, rgb8 = gs.probe_preview(grid, coeff, aov_samples=1, seed=P.SEED, vis=vis, moments=moments)
            fb, lin = got[u]
            assert (fb == _host(rgb8)).all() and (lin.view(np.uint32) == _host(rgb).view(np.uint32)).all(), f"frame {u}"
        assert (_host(age) == 3).all()
        assert not (got[0][0] == got[2][0]).all()
    finally:
        gs.close()


def test_rays_zero_is_the_frame_without_the_call(gpu):
    from rt_amd import scene as Sc
    sc = Sc.build_scene(4, W, H, 1, DEPTH)
    want8, want, _ = _full_frame(gpu, sc, 4)
    with Library(4) as lib:
        lib.host.rt_set_probe_update(0, HYST)
        for _ in range(2):   # (nothing is kept: the second call is the first again)
            fb, lin = lib.render(sc)
            assert fb.tobytes() == want8.tobytes() and lin.tobytes() == want.tobytes()
        lib.host.rt_set_probe_update(RAYS, HYST)
        lib.host.rt_set_scene_updates(0)   # without scene updates it does not apply either
        fb, lin = lib.render(sc)
        assert fb.tobytes() == want8.tobytes() and lin.tobytes() == want.tobytes()


def test_a_changed_reach_or_resolution_starts_over(gpu):
    from rt_amd import scene as Sc
    sc = Sc.build_scene(4, W, H, 1, DEPTH)
    with Library(4) as lib:
        lib.host.rt_set_probe_update(RAYS, HYST)
        first = lib.render(sc)
        want8, want, reach0 = _full_frame(gpu, sc, 4)
        assert first[0].tobytes() == want8.tobytes() and first[1].tobytes() == want.tobytes()   # a first call is the full bake
        _move(sc, LIGHT, 0.0, 25.0, 0.0)
        moved = lib.render(sc)
        want8, want, reach1 = _full_frame(gpu, sc, 4)
        assert reach1 != reach0, "the move must change the reach: this test is about the fall-back"
        assert moved[0].tobytes() == want8.tobytes() and moved[1].tobytes() == want.tobytes()
        lib.host.rt_set_probe_visibility(2)   # another resolution: the full bake again, not a round
        other = lib.render(sc)
        want8, want, _ = _full_frame(gpu, sc, 2)
        assert other[0].tobytes() == want8.tobytes() and other[1].tobytes() == want.tobytes()
        sc.objects[INNER].flags = sc.objects[INNER].flags ^ 1   # another scene: rebuilt, and the full bake
        rebuilt = lib.render(sc)
        want8, want, _ = _full_frame(gpu, sc, 2)
        assert rebuilt[0].tobytes() == want8.tobytes() and rebuilt[1].tobytes() == want.tobytes()

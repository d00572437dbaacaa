"""What the rooms of tests/dir_park_scenes.py are, from the oracle alone.

tests/test_gpu_dir_park.py renders one room per swapping pooled kernel (PARK_ROWS) to drive the retry stack of the direction
rounds until it meets the waiting list from above.  That only happens in a scene whose paths are deep and whose hits are
nearly all diffuse; here the oracle's own frame of each room (the very scene the device renders: one 8 x 8 tile, 64 spp,
depth 16) is held against conditions fixed beforehand:

  - the frame is finite;
  - rays > 12 x width x height x samples in the rooms without glass (a path of depth 16 that never ends early casts 17; the
    plain room keeps the existing test's bar of 15; twelve leaves room for the checker's halved albedo and the extra balls);
  - a glass room casts more rays than the all-diffuse room of its row (the second children add theirs), and so passes the bar;
  - the class of each room names its row of the pick table (rt_hip_kernel_for_class, as tests/test_pick_table.py asks it).

Were a room's count lower than the bar, its albedos would have to rise: the bar stays.
"""
import ctypes as C

import numpy as np
import pytest

from conftest import SEED
from dir_park_scenes import DEEP_GLASS_DEPTH, KERNELS, NO_GLASS, PARK_ROWS, REFR_SCENES, SCENES
from test_views_cpu import scene_class

_FRAMES = {}


def frame(pt, name):
    """the oracle's frame and counters of a scene, computed once per session and left unchanged"""
    if name not in _FRAMES:
        sc = SCENES[name]()
        mean, _, st = pt.render_pixels(sc, SEED)
        mean.setflags(write=False)
        _FRAMES[name] = (mean, dict(st), sc.width * sc.height * sc.samples)
        sc.free()
    return _FRAMES[name]


def test_one_room_per_swapping_kernel():
    kernels = [k for _, k, _ in PARK_ROWS]
    assert len(set(kernels)) == len(kernels) == 13 and len({n for n, _, _ in PARK_ROWS}) == 13
    assert all(KERNELS[n] == k for n, k, _ in PARK_ROWS)
    assert sorted(REFR_SCENES) == sorted(NO_GLASS) and len(REFR_SCENES) == 3
    for name, _, _ in PARK_ROWS:
        sc = SCENES[name]()
        assert (sc.width, sc.height, sc.samples, sc.max_depth) == (8, 8, 64, 16), name
        assert sc.n_triangles <= 40
        sc.free()


@pytest.mark.parametrize("name,kernel", [(n, k) for n, k, _ in PARK_ROWS], ids=[k for _, k, _ in PARK_ROWS])
def test_the_room_s_class_names_its_row(name, kernel):
    from rt_amd import abi
    sc = SCENES[name]()
    assert abi.load_shim().rt_hip_kernel_for_class(C.byref(scene_class(sc, "path", 0))).decode() == kernel
    sc.free()


@pytest.mark.parametrize("name", [n for n, _, _ in PARK_ROWS] + ["ragged_chk", "ragged_refr", "passes_refr", "passes_mem_s"])
def test_the_oracle_s_frame_is_finite_and_its_paths_are_deep(pt, name):
    mean, st, n_samples = frame(pt, name)
    assert np.isfinite(mean).all(), name
    print(name, "rays per sample", st["rays"] / n_samples)
    if name == "diffuse_room":
        assert st["rays"] > 15 * n_samples, st
    assert st["rays"] > 12 * n_samples, (name, st)


@pytest.mark.parametrize("name", REFR_SCENES)
def test_a_glass_room_casts_more_rays_than_the_diffuse_room_of_its_row(pt, name):
    _, st, n = frame(pt, name)
    _, st0, n0 = frame(pt, NO_GLASS[name])
    assert n == n0 and st["rays"] > st0["rays"] > 12 * n0, (name, st, st0)


def test_the_deep_glass_room(pt):
    """32 spp at a depth past 16 (bit 4 of the entry's 6-bit depth field); in one chunk its windowed sums do not fit, so its
    class is the static kernel's -- the GPU test takes the chunk count from the shim and asserts the pooled kernel there"""
    from rt_amd import abi
    sc = SCENES["deep_glass"]()
    assert sc.samples == 32 and 16 < sc.max_depth == DEEP_GLASS_DEPTH <= 28
    cls = scene_class(sc, "path", 0)
    assert abi.load_shim().rt_hip_kernel_for_class(C.byref(cls)).decode() == "pt_render_tiles_refr"
    cls.samples_per_chunk = 8
    assert abi.load_shim().rt_hip_kernel_for_class(C.byref(cls)).decode() == "pt_render_tiles_refr_pool"
    sc.free()
    mean, st, n = frame(pt, "deep_glass")
    _, st0, n0 = frame(pt, "diffuse_room")
    assert np.isfinite(mean).all()
    assert st["rays"] * n0 > st0["rays"] * n, (st, st0)    # rays per sample beyond the 16-deep plain room's

"""Pixel sums at the edges of what the library accepts (rt_hip_shim.hip: material_ok -- colours in [0, 1e100], |emission| <=
1e100): emitters of 1e3 .. 1e38, negative emission, colours of maximum 0 or above 1, the most samples and the deepest paths.
Every frame is compared with the oracle at an ABSOLUTE floor of 1e-9 that does not follow the scene's emitters: a launch must
not return a pixel that its pixel sums quantised (the fixed-point scale is set by the brightest emitter, reachable or not --
pt_device.h, pt_fixed_sums_fit).  Each case also names the body that rendered it.
"""
import numpy as np
import pytest

from conftest import SEED
from accum_range_scenes import (_custom, _fixed_point_fits, _parts, colour_scene, hidden_emitter_scene, negative_emission_scene,
                                visible_emitter_scene)
from util import assert_parity, class_scene

pytestmark = pytest.mark.gpu

FLOOR = 1e-9  # absolute; NOT fixed_point_floor(): the bar must not grow with the brightest emitter
HIDDEN_E = [1e3, 1e6, 1e9, 1e12, 1e15, 1e30]


@pytest.fixture(scope="module")
def gpu():
    import torch
    from rt_amd import abi, gpu as G
    assert abi.load_shim().rt_hip_device_count() >= 1, "no HIP device: the GPU tests must run on the GPU box"
    assert torch.cuda.is_available()
    return G


def _oracle(pt, ref, sc, seed=SEED):
    """the compiled reference (depth 5, spheres only) where it applies, else the oracle's restatement"""
    if ref is not None and sc.n_meshes == 0 and sc.max_depth == 5:
        return ref(5).render_pixels(sc, seed)
    return pt.render_pixels(sc, seed)


def _render_and_compare(gpu, pt, ref, sc, kernel, what, hdr=False, seed=SEED):
    gs = gpu.GpuScene(sc)
    img, img8, st = gs.render_image(seed)
    name = gs.last_launch_kernel()
    gs.close()
    mean, rgb8, ost = _oracle(pt, ref, sc, seed)
    assert st["samples"] == sc.width * sc.height * sc.samples
    assert_parity(img.cpu().numpy(), img8.cpu().numpy(), st, mean, rgb8, ost, what=what, hdr=hdr, abs_floor=FLOOR)
    assert name == kernel, f"{what}: rendered by {name}, expected {kernel}"
    return img


# the fixed-point bodies a scene class reaches, and where the same class goes once its sums need no bound (pt_pick_table's REFR rows)
BODIES = [
    ("tiles", dict(), "pt_render_tiles", "pt_render_tiles_refr_pool"),
    ("chk", dict(chk=True), "pt_render_tiles_chk", "pt_render_tiles_refr_pool"),
    ("tri", dict(tris=12), "pt_render_tiles_tri", "pt_render_tiles_tri_refr_pool"),
    ("pool_mem_s", dict(n_packed=120), "pt_render_tiles_pool_mem_s", "pt_render_tiles_refr_pool_mem"),
    ("pool_mem", dict(n_packed=300, wide=True), "pt_render_tiles_pool_mem", "pt_render_tiles_mem"),
    ("tri_queued", dict(tris=600), "pt_render_tiles_tri_queued", "pt_render_tiles_tri_queued_refr"),
    ("tri_queued_sph", dict(tris=600, round_mesh=True), "pt_render_tiles_tri_queued_sph", "pt_render_tiles_tri_queued_refr_sph"),
]


@pytest.mark.parametrize("E", HIDDEN_E, ids=[f"E={e:g}" for e in HIDDEN_E])
@pytest.mark.parametrize("body,cls,fixed,unbounded", BODIES, ids=[b[0] for b in BODIES])
def test_hidden_emitter_does_not_quantise_the_frame(gpu, pt, ref, body, cls, fixed, unbounded, E):
    """a room whose brightest emitter is sealed inside an opaque shell renders as the room without it"""
    sc = hidden_emitter_scene(E, **cls)
    # the test's own premise: no ray reaches the emitter, so the oracle's frame with it is the frame with it switched off
    objs, meshes = _parts(sc)
    objs[-1]["emission"] = (0.0, 0.0, 0.0)
    dark = _custom(objs, meshes, sc.width, sc.height, sc.samples, sc.max_depth)
    m1, b1, s1 = pt.render_pixels(sc, SEED)
    m0, b0, s0 = pt.render_pixels(dark, SEED)
    assert np.array_equal(m1, m0) and np.array_equal(b1, b0) and s1 == s0, "the shell leaks: the test's scene is wrong"
    kernel = fixed if _fixed_point_fits(sc, E) else unbounded
    _render_and_compare(gpu, pt, ref, sc, kernel, f"{body}, hidden emitter {E:g}")


GLASS_HIDDEN = [
    # windowed sums (the pooled refraction forms), and fp64 sums (the static form) once a term can reach 2^128
    ("spheres", dict(refr=True), 1e9, "pt_render_tiles_refr_pool"),
    ("spheres", dict(refr=True), 1e38, "pt_render_tiles_refr"),
    ("small mesh", dict(refr=True, tris=12), 1e15, "pt_render_tiles_tri_refr_pool"),
    ("hierarchy", dict(refr=True, tris=600), 1e12, "pt_render_tiles_tri_queued_refr"),
    ("plain room", dict(), 1e38, "pt_render_tiles_refr"),
]


@pytest.mark.parametrize("what,cls,E,kernel", GLASS_HIDDEN, ids=[f"{g[0]}-{g[2]:g}" for g in GLASS_HIDDEN])
def test_hidden_emitter_with_glass(gpu, pt, ref, what, cls, E, kernel):
    sc = hidden_emitter_scene(E, **cls)
    _render_and_compare(gpu, pt, ref, sc, kernel, f"{what}, hidden emitter {E:g}")


@pytest.mark.parametrize("E", [1e6, 1e9])
def test_visible_bright_emitter(gpu, pt, ref, E):
    """a small emitter of E in view beside the dim room: the bar scales with the brightest pixel (hdr), not with E"""
    sc = visible_emitter_scene(E)
    _render_and_compare(gpu, pt, ref, sc, "pt_render_tiles_refr_pool", f"visible emitter {E:g}", hdr=True)


NEGATIVE = [
    ("fixed point", dict(), "pt_render_tiles"),
    ("fixed point, parked walks", dict(tris=600, chk=True), "pt_render_tiles_tri_queued_chk"),
    ("windowed", dict(refr=True), "pt_render_tiles_refr_pool"),
    ("static", dict(refr=True, max_depth=30), "pt_render_tiles_refr"),   # 2^31 x 4 spp: past the windows' capacity
]


@pytest.mark.parametrize("what,cls,kernel", NEGATIVE, ids=[n[0] for n in NEGATIVE])
def test_negative_emission(gpu, pt, ref, what, cls, kernel):
    sc = negative_emission_scene(**cls)
    _render_and_compare(gpu, pt, ref, sc, kernel, f"negative emission, {what}")


COLOURS = [
    ("checker", dict(chk=True), "pt_render_tiles_chk"),
    ("plain", dict(), "pt_render_tiles_chk"),          # the scene's own M_CHECKERED spheres
    ("small mesh", dict(tris=12), "pt_render_tiles_tri_chk"),
    ("windowed", dict(refr=True), "pt_render_tiles_refr_pool"),
]


@pytest.mark.parametrize("what,cls,kernel", COLOURS, ids=[c[0] for c in COLOURS])
def test_colours_at_the_edges(gpu, pt, ref, what, cls, kernel):
    _render_and_compare(gpu, pt, ref, colour_scene(**cls), kernel, f"edge colours, {what}")


def test_many_samples_the_sum_bound_decides_the_scale(gpu, pt, ref):
    """16 x 8 at 4096 spp: samples x per-sample bound < 2^62 sets the scale (beyond 2^11 samples), not the term's 2^51"""
    objs, meshes = _parts(class_scene(width=16, height=8, samples=4096, depth=5))
    sc = _custom(objs, meshes, 16, 8, 4096, 5)
    assert sc.samples > 2 ** 11
    _render_and_compare(gpu, pt, ref, sc, "pt_render_tiles", "4096 spp")


@pytest.mark.parametrize("E,kernel", [(None, "pt_render_tiles"), (1e6, "pt_render_tiles_refr")])
def test_depth_200_without_glass(gpu, pt, ref, E, kernel):
    """200 bounces: the room's own lights keep fixed-point sums; a hidden emitter of 1e6 sends it to the fp64 sums of the static
    kernel (the windowed forms end at depth 29), whose pending-ray stacks are never pushed without M_REFRACTION"""
    if E is None:
        objs, meshes = _parts(class_scene(width=24, height=16, samples=4, depth=200))
        sc = _custom(objs, meshes, 24, 16, 4, 200)
    else:
        sc = hidden_emitter_scene(E, width=24, height=16, samples=4, max_depth=200)
    _render_and_compare(gpu, pt, ref, sc, kernel, f"depth 200, {E}")


def test_glass_at_the_deepest_depth_with_chunks(gpu, pt):
    """M_REFRACTION at PT_REFRACT_MAX_DEPTH, rendered in sample chunks: the same frame as the oracle's"""
    import torch
    sc = class_scene(refr=True, width=24, height=16, samples=8, depth=32)
    gs = gpu.GpuScene(sc)
    count = gpu.n_tiles(sc.width, sc.height)
    t, t8, s = gs.render_tiles(SEED, 0, 1, count, chunks=4)
    name = gs.last_launch_kernel()
    img = torch.zeros((sc.height, sc.width, 3), dtype=torch.float32, device=t.device)
    img8 = torch.zeros((sc.height, sc.width, 3), dtype=torch.uint8, device=t.device)
    gs.untile(t, t8, 0, 1, count, img, img8)
    torch.cuda.synchronize()
    gs.launch_status()
    gs.close()
    mean, rgb8, ost = pt.render_pixels(sc, SEED)
    from rt_amd import abi
    st = s.cpu().tolist()
    st = dict(rays=st[abi.STAT_RAYS], tests=st[abi.STAT_TESTS], casts=st[abi.STAT_CASTS])
    assert_parity(img.cpu().numpy(), img8.cpu().numpy(), st, mean, rgb8, ost, what="glass, depth 32, 4 chunks", abs_floor=FLOOR)
    assert name == "pt_render_tiles_refr", name


def test_two_by_two_image(gpu, pt, ref):
    objs, meshes = _parts(class_scene(width=2, height=2, samples=16, depth=5))
    _render_and_compare(gpu, pt, ref, _custom(objs, meshes, 2, 2, 16, 5), "pt_render_tiles", "2 x 2")


@pytest.mark.parametrize("which", ["bright", "negative"])
def test_partition_and_chunks_are_bit_invariant(gpu, which):
    """tiles over three ranks, and samples in chunks, give the one-launch frame bit for bit"""
    import torch
    sc = hidden_emitter_scene(1e9, width=40, height=24, samples=16) if which == "bright" else \
        negative_emission_scene(width=40, height=24, samples=16)
    gs = gpu.GpuScene(sc)
    full, full8, st = gs.render_image(SEED)
    world = 3
    image, image8 = torch.zeros_like(full), torch.zeros_like(full8)
    for r in range(world):
        first, stride, count = gpu.rank_tiles(sc.width, sc.height, r, world)
        t, t8, _ = gs.render_tiles(SEED, first, stride, count)
        gs.untile(t, t8, first, stride, count, image, image8)
    torch.cuda.synchronize()
    assert torch.equal(image, full) and torch.equal(image8, full8), "tile partition"
    count = gpu.n_tiles(sc.width, sc.height)
    for chunks in (2, 5, 16):
        image, image8 = torch.zeros_like(full), torch.zeros_like(full8)
        t, t8, _ = gs.render_tiles(SEED, 0, 1, count, chunks=chunks)
        gs.untile(t, t8, 0, 1, count, image, image8)
        torch.cuda.synchronize()
        assert torch.equal(image, full) and torch.equal(image8, full8), f"{chunks} sample chunks"
    gs.launch_status()
    gs.close()

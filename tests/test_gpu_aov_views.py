"""Every AOV form (pt_aov_tiles*) under other cameras, and with its scene far out or scaled (util.VARIANTS).

render_aov is its own instantiation of the scan (no tile-cull list, its own use of the triangles' bounding ball) over the tables
the beauty kernels read -- near_R2, the packed-fp32 filter widened by e (|c| + near_R), tri32, the leading walls' pruning, the
hierarchy -- and adds what only it has: the sphere normal through rcp / sqrt at scales 1e-3 .. 1e22, depth = (float)t_min,
the strict-< object pick, the last passing triangle's (u, v).  Here each class of util.AOV_FORM_CLASSES renders at
util.AOV_VIEW_SIZE through the inside, steep, telephoto, wide, sheared and near_plane cameras and with its scene moved 2e7
out or scaled by 1e-3 and 1e3; all five buffers of the whole image equal the expectation built from the compiled reference
(tests/aov_expected.py) bit for bit, no pixel left out.  tests/test_aov_views_cpu.py shows what those frames hold.  The form
each launch takes is the one util.AOV_MOVES states.  Then: tile subsets under a hand-built camera, the image entry point on a
logical device of a device map, and -- last -- the tally: every form compared under at least 8 of the 9 variants.
"""
import ctypes as C

import numpy as np
import pytest

from aov_expected import expected_image, mismatch
from conftest import SEED
from util import AOV_FORM_CLASSES, AOV_VIEW_SIZE, VARIANTS, aov_form_under, aov_view_scene, class_scene, view_variant

pytestmark = pytest.mark.gpu

TALLY = {}   # form -> [(variant, class's form, launches of the form after the comparison)]


@pytest.fixture(scope="module")
def gpu():
    import torch
    from rt_amd import abi, gpu as G
    assert abi.load_shim().rt_hip_device_count() >= 1, "no HIP device: the GPU tests must run on the GPU box"
    assert torch.cuda.is_available()
    yield G
    abi.load_shim().rt_hip_set_device_map(None, 0)


def _launches(form):
    from rt_amd import abi
    shim = abi.load_shim()
    for k in range(shim.rt_hip_aov_kernel_count()):
        n = C.c_uint64(0)
        if shim.rt_hip_aov_kernel_launches(k, C.byref(n)).decode() == form:
            return n.value
    raise KeyError(form)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("form,cls", AOV_FORM_CLASSES, ids=[f for f, _ in AOV_FORM_CLASSES])
def test_every_form_equals_the_reference_under_every_variant(gpu, ref_mesh, form, cls, variant):
    S = AOV_VIEW_SIZE["samples"]
    sc = aov_view_scene(cls, variant)
    takes = aov_form_under(form, variant)
    gs = gpu.GpuScene(sc)
    assert gs.aov_kernel_name() == takes, f"{form} {variant}: the scene takes {gs.aov_kernel_name()}, AOV_MOVES says {takes}"
    before = _launches(takes)
    got = gs.aov_image(SEED, S)
    after = _launches(takes)
    assert after == before + 1, f"{form} {variant}: {after - before} launches of {takes}"
    assert got["hits"].shape == (AOV_VIEW_SIZE["height"], AOV_VIEW_SIZE["width"])
    msg = mismatch(got, expected_image(ref_mesh(5), sc, SEED, S))
    assert not msg, f"{takes} ({cls}) {variant}: {msg}"
    TALLY.setdefault(takes, []).append((variant, form, after))
    gs.close()
    sc.free()


@pytest.mark.parametrize("cls", [dict(n_packed=4), dict(n_packed=4, tris=40, mesh_chk=True), dict(n_packed=4, tris=400, chk=True),
                                 dict(n_packed=300, tris=60)], ids=["spheres", "flat_mesh_chk", "hierarchy_chk", "mem"])
def test_tile_subsets_under_a_hand_built_camera(gpu, ref_mesh, cls):
    """the sheared variant (rolled, mirrored, V sheared, principal ray outside the frame) at 37 x 21: launches of tile subsets
    give the full launch's tiles, and their untiled union is the reference's image"""
    import torch
    from rt_amd import abi
    W, H, S = 37, 21, 2
    sc = aov_view_scene(cls, "sheared", width=W, height=H, samples=S)
    gs = gpu.GpuScene(sc)
    total = gpu.n_tiles(W, H)
    full = gs.render_aov(SEED, S)
    torch.cuda.synchronize()
    img = {f: np.zeros((H, W, 3) if abi.AOV_CHANNELS[f] == 3 else (H, W), np.uint32) for f in abi.AOV_FIELDS}
    for first, stride, count in ((1, 3, (total - 1 + 2) // 3), (0, 3, (total + 2) // 3), (2, 3, (total - 2 + 2) // 3),
                                 (0, 1, 5), (4, 2, 3), (total - 1, 1, 1)):
        part = gs.render_aov(SEED, S, first, stride, count)
        torch.cuda.synchronize()
        for f in abi.AOV_FIELDS:
            a, b = part[f][:count].cpu().numpy(), full[f][first:first + stride * count:stride].cpu().numpy()
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (f, first, stride, count)
        if stride == 3:
            sub = gs.untile_aov(part, first, stride, count)
            torch.cuda.synchronize()
            for f in abi.AOV_FIELDS:
                img[f] |= sub[f].cpu().numpy().view(np.uint32)   # disjoint tile sets; zeros elsewhere
    got = {f: img[f].view(np.float32) if f in ("albedo", "normal", "depth") else img[f] for f in abi.AOV_FIELDS}
    msg = mismatch(got, gs.aov_image(SEED, S))
    assert not msg, f"untiled subsets {cls}: {msg}"
    msg = mismatch(got, expected_image(ref_mesh(5), sc, SEED, S))
    assert not msg, f"sheared, ragged {cls}: {msg}"
    gs.close()
    sc.free()


def test_the_image_entry_point_on_a_logical_device(gpu, ref_mesh):
    """rt_hip_render_aov_image(..., device=2, ...) under the device map (0, 0, 0): device 0's buffers bit for bit, and the
    reference's; without the map, logical device 2 does not exist here"""
    from rt_amd import abi
    shim = abi.load_shim()
    S = 2
    sc = view_variant(class_scene(n_packed=4, tris=40, mesh_chk=True, width=40, height=24, samples=S), "sheared")
    assert shim.rt_hip_set_device_map(None, 0) == 0
    zero = gpu.aov_image_host(sc, SEED, S, device=0)
    arr = (C.c_int * 3)(0, 0, 0)
    assert shim.rt_hip_set_device_map(arr, 3) == 0, shim.rt_hip_last_error()
    try:
        two = gpu.aov_image_host(sc, SEED, S, device=2)
        with pytest.raises(gpu.ShimError):
            gpu.aov_image_host(sc, SEED, S, device=3)   # beyond the map
    finally:
        shim.rt_hip_set_device_map(None, 0)
    msg = mismatch(two, zero)
    assert not msg, f"logical device 2 of (0, 0, 0) against device 0: {msg}"
    msg = mismatch(two, expected_image(ref_mesh(5), sc, SEED, S))
    assert not msg, msg
    sc.free()


def test_zz_every_form_was_compared_under_at_least_eight_variants(gpu):
    """last in this file: the tally of the comparisons above that passed, by the form the launch took (a launch that
    AOV_MOVES moves counts for the form it took, not for its class's)"""
    from rt_amd import abi
    shim = abi.load_shim()
    forms = [shim.rt_hip_aov_kernel_launches(k, None).decode() for k in range(shim.rt_hip_aov_kernel_count())]
    assert sorted(forms) == sorted(f for f, _ in AOV_FORM_CLASSES)
    print("\nAOV form x variant: whole images (%d x %d, %d samples) equal to the reference bit for bit" %
          (AOV_VIEW_SIZE["width"], AOV_VIEW_SIZE["height"], AOV_VIEW_SIZE["samples"]))
    print("  %-26s %s  own  moved in" % ("form", " ".join("%-10s" % v for v in VARIANTS)))
    short = []
    for form in forms:
        rows = TALLY.get(form, [])
        own = {v for v, f, _ in rows if f == form}
        moved_in = [f"{f}:{v}" for v, f, _ in rows if f != form]
        print("  %-26s %s  %3d  %s" % (form, " ".join("%-10s" % ("ok" if v in own else "-") for v in VARIANTS), len(own),
                                        ", ".join(moved_in)))
        if len(own) < 8 or not own >= set(VARIANTS) - {"tiny"}:
            short.append((form, sorted(own)))
    assert not short, f"forms compared under fewer than 8 variants of their own class: {short}"
    assert sum(len(r) for r in TALLY.values()) == len(AOV_FORM_CLASSES) * len(VARIANTS)

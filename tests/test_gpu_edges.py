"""Every row of the kernel pick table at ragged image sizes, on tile subsets, in uneven sample chunks and in passes.

The row test of tests/test_gpu_parity.py renders each member at 48 x 32: whole 8 x 8 tiles only, one launch, the suggested
chunks.  Here the same scenes (util.class_scene, resized through sc.width / sc.height / sc.samples, so that geometry, camera
and pick stay the row's) go where tile kernels usually go wrong:

  A  47 x 25, 7 spp: a right column of tiles 7 pixels wide, a bottom row 1 pixel high, a corner tile of 7 pixels
  B  65 x 2, 5 spp:  one row of tiles 2 pixels high, the last one 1 x 2
  C  2 x 41, 3 spp:  one column of tiles 2 pixels wide, the last one 2 x 1

Per row: the oracle's frame at A, B and C; the padding pixels of edge tiles (outside the image) exactly 0; chunk counts 1, 3
and 7 bit for bit; strided and contiguous tile subsets bit for bit against the whole frame, by tile index (padding
included); passes of 2 + 5 samples, the oracle's frame after the first and the one-shot frame after the last.  Then NaN
samples across passes, and rt_hip_accum_read_image over a tile subset.  The GPU tests carry the gpu marker one by one: the
shape test at the end runs without a GPU.
"""
import contextlib

import numpy as np
import pytest

from conftest import SEED
from test_gpu_parity import PICK_ROWS, _WP
from util import acc_scale_exp, assert_parity, fixed_point_floor, untile_numpy

TILE = 8
SHAPES = {"A": (47, 25, 7), "B": (65, 2, 5), "C": (2, 41, 3)}   # width, height, samples per pixel
ROW_IDS = [f"{k}:{i}:{'+'.join(f'{a}={b}' for a, b in c.items())}{':fault%d' % f if f else ''}" for c, i, f, k in PICK_ROWS]


@pytest.fixture(scope="module")
def gpu():
    import torch
    from rt_amd import abi, gpu as G
    assert abi.load_shim().rt_hip_device_count() >= 1, "no HIP device: the GPU tests must run on the GPU box"
    assert torch.cuda.is_available()
    return G


def edge_classes(width, height):
    """the tile rule (8 x 8 tiles, row-major, the last column / row cut at the image's edge) -> what the edges of the image are"""
    tx, ty = (width + TILE - 1) // TILE, (height + TILE - 1) // TILE
    last_w, last_h = width - TILE * (tx - 1), height - TILE * (ty - 1)
    return dict(tiles=tx * ty, tiles_x=tx, tiles_y=ty, last_col_w=last_w, last_row_h=last_h, corner_pixels=last_w * last_h)


def _outside(width, height, tiles):
    """[len(tiles), 64] bool: pixel t of each tile lies outside the image (row-major inside the tile)"""
    tx = (width + TILE - 1) // TILE
    t = np.arange(TILE * TILE)
    out = []
    for tile in tiles:
        x0, y0 = (tile % tx) * TILE, (tile // tx) * TILE
        out.append((x0 + (t & 7) >= width) | (y0 + (t >> 3) >= height))
    return np.array(out)


def _assert_padding_zero(t, t8, width, height, tiles, what):
    """every pixel of an edge tile outside the image is exactly 0.0 (all 32 bits) in f32 and 0 in u8"""
    out = _outside(width, height, tiles)
    assert out.any(), "the shape should have padding pixels"
    f = np.asarray(t)[: len(tiles)].view(np.uint32)
    b = np.asarray(t8)[: len(tiles)]
    assert not f[out].any(), f"{what}: {int((f[out] != 0).any(axis=1).sum())} padding pixels not 0.0 in f32"
    assert not b[out].any(), f"{what}: {int((b[out] != 0).any(axis=1).sum())} padding pixels not 0 in u8"


@contextlib.contextmanager
def _faults(shim, faults):
    """the row's allocation faults (as the row test of test_gpu_parity.py), reset whatever happens"""
    if faults & _WP:
        shim.rt_hip_release_cache()      # no pending-ray pool yet: the launch has to ask for the wide one
    shim.rt_hip_selftest_fail_alloc(faults)
    try:
        yield
    finally:
        shim.rt_hip_selftest_fail_alloc(0)


def _shaped(cls, shape):
    from util import class_scene
    sc = class_scene(**cls)
    sc.width, sc.height, sc.samples = SHAPES[shape]
    return sc


def _tiles(gs, kernel, first, stride, count, chunks, integrator):
    import torch
    t, t8, st = gs.render_tiles(SEED, first, stride, count, chunks=chunks, integrator=integrator)
    assert gs.last_launch_kernel() == kernel, (first, stride, count, chunks, gs.last_launch_kernel())
    torch.cuda.synchronize()
    return t.cpu().numpy(), t8.cpu().numpy(), st.cpu().tolist()


def _stats(st):
    return dict(zip(("rays", "casts", "tests", "samples"), st))


@pytest.mark.gpu
@pytest.mark.parametrize("cls,integrator,faults,kernel", PICK_ROWS, ids=ROW_IDS)
def test_ragged_shapes_render_the_oracle_s_frame(gpu, pt, cls, integrator, faults, kernel):
    """check 1: shapes A, B and C whole (render_image), pixel by pixel and counter by counter against the oracle"""
    from rt_amd import abi
    shim = abi.load_shim()
    sc = _shaped(cls, "A")
    got = {}
    with _faults(shim, faults):
        gs = gpu.GpuScene(sc)
        for shape in SHAPES:
            sc.width, sc.height, sc.samples = SHAPES[shape]
            img, img8, st = gs.render_image(SEED, integrator=integrator)
            assert gs.last_launch_kernel() == kernel, (shape, gs.last_launch_kernel())
            got[shape] = (img.cpu().numpy(), img8.cpu().numpy(), st)
    for shape, (img, img8, st) in got.items():
        sc.width, sc.height, sc.samples = SHAPES[shape]
        assert img.shape == (sc.height, sc.width, 3)
        assert st["samples"] == sc.width * sc.height * sc.samples, (shape, st)
        mean, rgb8, ost = pt.render_pixels(sc, SEED, integrator=integrator)
        assert_parity(img, img8, st, mean, rgb8, ost, what=f"{kernel} {cls} shape {shape}", hdr=True,
                      abs_floor=fixed_point_floor(sc))
    gs.close()
    sc.free()


@pytest.mark.gpu
@pytest.mark.parametrize("cls,integrator,faults,kernel", PICK_ROWS, ids=ROW_IDS)
def test_sample_chunks_and_tile_subsets_give_the_whole_frame_bit_for_bit(gpu, pt, cls, integrator, faults, kernel):
    """checks 2-4 at shape A: padding pixels exactly 0; 1, 3 (2 + 2 + 3) and 7 (one sample each) chunks bit for bit, counters
    equal; three strided subsets (first 0, 1, 2, stride 3) and a contiguous one (first 5, count 7) equal to the whole frame's
    tiles of the same index, the strided counters summing to the whole frame's.  The one-chunk frame is the oracle's."""
    from rt_amd import abi
    shim = abi.load_shim()
    sc = _shaped(cls, "A")
    w, h = sc.width, sc.height
    total = gpu.n_tiles(w, h)
    assert total == 24
    with _faults(shim, faults):
        gs = gpu.GpuScene(sc)
        frames = {c: _tiles(gs, kernel, 0, 1, total, c, integrator) for c in (1, 3, 7)}
        subsets = {(first, 3, 8): _tiles(gs, kernel, first, 3, 8, gs.suggest_chunks(8), integrator) for first in (0, 1, 2)}
        subsets[(5, 1, 7)] = _tiles(gs, kernel, 5, 1, 7, gs.suggest_chunks(7), integrator)
        gs.launch_status()
    whole_t, whole_t8, whole_st = frames[1]
    assert whole_st[3] == w * h * sc.samples
    for c, (t, t8, st) in frames.items():
        _assert_padding_zero(t, t8, w, h, range(total), f"{kernel}, {c} chunks")
        assert np.array_equal(t.view(np.uint32), whole_t.view(np.uint32)), f"{kernel}: {c} chunks differ from one"
        assert np.array_equal(t8, whole_t8), f"{kernel}: bytes of {c} chunks differ from one"
        assert st == whole_st, (kernel, c, st, whole_st)
    strided = np.zeros(4, dtype=np.int64)
    for (first, stride, count), (t, t8, st) in subsets.items():
        ids = [first + k * stride for k in range(count)]
        assert t.shape[0] == count and ids[-1] < total
        _assert_padding_zero(t, t8, w, h, ids, f"{kernel}, tiles {first}::{stride} x {count}")
        assert np.array_equal(t.view(np.uint32), whole_t[ids].view(np.uint32)), (kernel, first, stride, count)
        assert np.array_equal(t8, whole_t8[ids]), (kernel, first, stride, count)
        if stride == 3:
            strided += np.array(st)
    assert strided.tolist() == whole_st, (kernel, strided.tolist(), whole_st)
    img = untile_numpy(whole_t, w, h, 0, 1, total, np.zeros((h, w, 3), np.float32))
    img8 = untile_numpy(whole_t8, w, h, 0, 1, total, np.zeros((h, w, 3), np.uint8))
    mean, rgb8, ost = pt.render_pixels(sc, SEED, integrator=integrator)
    assert_parity(img, img8, _stats(whole_st), mean, rgb8, ost, what=f"{kernel} {cls} shape A, one chunk", hdr=True,
                  abs_floor=fixed_point_floor(sc))
    gs.close()
    sc.free()


@pytest.mark.gpu
@pytest.mark.parametrize("cls,integrator,faults,kernel", PICK_ROWS, ids=ROW_IDS)
def test_passes_at_a_ragged_size(gpu, pt, cls, integrator, faults, kernel):
    """check 5: shape A's budget of 7 in passes of 2 and 5, the faults still injected: after 2 samples the oracle's frame of 2
    (the floor of test_gpu_progressive.py's intermediate frames), after 7 the one-shot frame at the suggested chunks bit for bit,
    counters summed; padding 0 after each resolve (pt_resolve_tiles / pt_resolve_slices)"""
    import torch
    from rt_amd import abi
    shim = abi.load_shim()
    sc = _shaped(cls, "A")
    w, h, budget = sc.width, sc.height, sc.samples
    total = gpu.n_tiles(w, h)
    with _faults(shim, faults):
        gs = gpu.GpuScene(sc)
        one_t, one_t8, one_st = _tiles(gs, kernel, 0, 1, total, gs.suggest_chunks(total), integrator)
        acc = gs.accumulate(SEED, budget, integrator=integrator)
        assert acc.kernel == kernel
        stats = torch.zeros(4, dtype=torch.int64, device=torch.device("cuda", gs.device))
        resolved = []
        for n in (2, 5):
            acc.add(n, stats)
            assert acc.kernel == kernel
            t, t8 = acc.resolve()
            torch.cuda.synchronize()
            resolved.append((acc.samples, t.cpu().numpy(), t8.cpu().numpy(), stats.cpu().tolist()))
        gs.launch_status()
    (k2, t2, t82, st2), (k7, t7, t87, st7) = resolved
    assert (k2, k7) == (2, budget)
    for t, t8, k in ((t2, t82, k2), (t7, t87, k7)):
        _assert_padding_zero(t, t8, w, h, range(total), f"{kernel}, resolved after {k}")
    assert np.array_equal(t7.view(np.uint32), one_t.view(np.uint32)), f"{kernel}: passes 2 + 5 differ from the one-shot frame"
    assert np.array_equal(t87, one_t8), kernel
    assert st7 == one_st, (kernel, st7, one_st)
    img = untile_numpy(t2, w, h, 0, 1, total, np.zeros((h, w, 3), np.float32))
    img8 = untile_numpy(t82, w, h, 0, 1, total, np.zeros((h, w, 3), np.uint8))
    assert st2[3] == w * h * k2
    mean, rgb8, ost = pt.render_pixels(sc, SEED, spp=k2, integrator=integrator)
    floor = max(fixed_point_floor(sc), (sc.max_depth + 2) * 2.0 ** -acc_scale_exp(sc, budget) / 2)
    assert_parity(img, img8, _stats(st2), mean, rgb8, ost, what=f"{kernel} {cls} shape A after {k2} of {budget}", hdr=True,
                  abs_floor=floor)
    acc.close()
    gs.close()
    sc.free()


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["pooled", "pooled_chunks", "windowed", "static"])
def test_nan_samples_keep_poisoning_their_pixel_across_passes(gpu, form):
    """the NaN scene of test_gpu_parity.py's test_nan_samples_poison_the_pixel_in_every_kernel_family with a budget of 9 in
    passes of 1, 2, 4 and 2: the NaN pixels only grow from pass to pass (integer sums carry a NaN sample in the tile records'
    NaN masks, atomicOr; the static body in its fp64 slice sums), a NaN pixel is 255 in the bytes, and after the budget the
    frame is the one-shot frame (NaN where it is NaN).  pooled_chunks: the one-shot frame in two chunks; windowed: a glass
    sphere out of reach (M_REFRACTION's windowed sums); static: the same at max_depth 30, where no windowed sums fit (fp64 slice sums)"""
    import torch
    from rt_amd import abi, scene as S
    c = (1.0e9, 1.0e9, 1.0e9)
    objs = [dict(flags=abi.M_DEFAULT, radius=2.0e-8, center=c, color=(0.5, 0.4, 0.3), emission=(0.3, 0.2, 0.1)),
            dict(flags=abi.M_DEFAULT, radius=5.0, center=(0, 0, 0), color=(0.7, 0.7, 0.7))]
    if form in ("windowed", "static"):
        objs.append(dict(flags=abi.M_REFRACTION, radius=1.0, center=(-3.0e9, 5.0e9, 0), color=(0.9, 0.9, 0.9)))  # never reached
    budget, passes = 9, (1, 2, 4, 2)
    sc = S.custom_scene(objs, 24, 16, budget, 30 if form == "static" else 4, c, (0, 0, 0))
    gs = gpu.GpuScene(sc)
    total = gpu.n_tiles(24, 16)
    t, t8, st = gs.render_tiles(SEED, 0, 1, total, chunks=2 if form == "pooled_chunks" else gs.suggest_chunks(total))
    one_shot_kernel = gs.last_launch_kernel()
    expect = {"pooled": "pt_render_tiles", "pooled_chunks": "pt_render_tiles", "windowed": "pt_render_tiles_refr_pool",
              "static": "pt_render_tiles_refr"}[form]
    assert one_shot_kernel == expect, one_shot_kernel
    acc = gs.accumulate(SEED, budget)
    assert acc.kernel == expect
    stats = torch.zeros(4, dtype=torch.int64, device="cuda")
    frames = []
    for n in passes:
        acc.add(n, stats)
        at, at8 = acc.resolve()
        torch.cuda.synchronize()
        frames.append((acc.samples, at.cpu().numpy(), at8.cpu().numpy()))
    gs.launch_status()
    one, one8 = t.cpu().numpy(), t8.cpu().numpy()
    nan_before = np.zeros(one.shape, dtype=bool)
    for k, f, f8 in frames:
        nan = np.isnan(f)
        assert (nan | ~nan_before).all(), f"{form}: a NaN pixel turned finite after {k} samples"
        assert (f8[nan] == 255).all(), (form, k)
        nan_before = nan
    assert nan_before.any() and not nan_before.all(), "the scene should give both NaN and finite pixels"
    assert np.isnan(frames[1][1]).any(), "NaN samples should come before the last pass (the parity test's frame of 2 has them)"
    assert np.array_equal(frames[-1][1], one, equal_nan=True), form
    assert np.array_equal(frames[-1][2], one8), form
    assert stats.cpu().tolist() == st.cpu().tolist()
    acc.close()
    gs.close()
    sc.free()


READ_ROWS = [r for r in PICK_ROWS if r[3] in ("pt_render_tiles", "pt_render_tiles_refr_pool", "pt_render_tiles_refr", "pt_whitted_tiles")]


@pytest.mark.gpu
@pytest.mark.parametrize("cls,integrator,faults,kernel", READ_ROWS, ids=[f"{k}:{i}" for _, i, _, k in READ_ROWS])
def test_read_image_of_an_accumulation_over_a_tile_subset(gpu, pt, cls, integrator, faults, kernel):
    """rt_hip_accum_read_image of an accumulation of shape A over tiles 1, 4, 7, ... (first 1, stride 3, 8 tiles), on each sum
    form -- fixed point, windowed, static fp64 slices (trace_path at max_depth 30, cast_ray) --, after 2 and after all 7
    samples: the subset's pixels are untile(resolve()), every other pixel is 0 (rt_hip.h), the return code 0; after the whole
    budget the subset's pixels are the oracle's"""
    import torch
    from rt_amd import abi
    from util import tile_pixels
    assert not faults
    shim = abi.load_shim()
    sc = _shaped(cls, "A")
    w, h, budget = sc.width, sc.height, sc.samples
    first, stride, count = 1, 3, 8
    ids = [first + k * stride for k in range(count)]
    gs = gpu.GpuScene(sc)
    acc = gs.accumulate(SEED, budget, integrator=integrator, first=first, stride=stride, count=count)
    assert acc.kernel == kernel
    inside = np.zeros((h, w), dtype=bool)
    inside.reshape(-1)[tile_pixels(w, h, ids)] = True
    for n in (2, 5):
        acc.add(n)
        t, t8 = acc.resolve()
        torch.cuda.synchronize()
        img = np.full((h, w, 3), -1.0, dtype=np.float32)   # what read_image does not write stays -1 / 7
        img8 = np.full((h, w, 3), 7, dtype=np.uint8)
        assert shim.rt_hip_accum_read_image(acc.handle, img.ctypes.data, img8.ctypes.data) == 0, shim.rt_hip_last_error()
        want = untile_numpy(t.cpu().numpy(), w, h, first, stride, count, np.zeros((h, w, 3), np.float32))
        want8 = untile_numpy(t8.cpu().numpy(), w, h, first, stride, count, np.zeros((h, w, 3), np.uint8))
        assert np.array_equal(img.view(np.uint32), want.view(np.uint32)) and np.array_equal(img8, want8), (kernel, acc.samples)
        assert not img.view(np.uint32)[~inside].any() and not img8[~inside].any(), (kernel, acc.samples)
        assert img[inside].any(), "the subset should not be black"
    assert acc.samples == budget
    px = tile_pixels(w, h, ids)
    mean, rgb8, _ = pt.render_pixels(sc, SEED, pixels=px, integrator=integrator)
    assert_parity(img.reshape(-1, 3)[px], img8.reshape(-1, 3)[px], None, mean, rgb8, None,
                  what=f"{kernel} read_image of tiles {first}::{stride}", hdr=True, abs_floor=fixed_point_floor(sc))
    acc.close()
    gs.close()
    sc.free()


def test_the_shapes_reach_ragged_edges():
    """the shapes above stay ragged: a later edit must not round them to whole tiles (CPU, the tile rule alone)"""
    from rt_amd.dist import n_tiles
    a, b, c = (edge_classes(*SHAPES[s][:2]) for s in "ABC")
    assert (a["last_col_w"], a["last_row_h"], a["corner_pixels"], a["tiles"]) == (7, 1, 7, 24)
    assert (b["tiles_y"], b["last_row_h"], b["last_col_w"]) == (1, 2, 1)
    assert (c["tiles_x"], c["last_col_w"], c["last_row_h"]) == (1, 2, 1)
    for s, (w, h, spp) in SHAPES.items():
        e = edge_classes(w, h)
        assert e["tiles"] == n_tiles(w, h)
        assert w % TILE and h % TILE, f"shape {s} is tile-aligned in a dimension"
        assert _outside(w, h, range(e["tiles"])).sum() == e["tiles"] * TILE * TILE - w * h
    # the chunk counts of check 3 split shape A's samples unevenly (2 + 2 + 3) and one sample each
    spp = SHAPES["A"][2]
    assert [(k + 1) * spp // 3 - k * spp // 3 for k in range(3)] == [2, 2, 3]
    assert spp == 7
    # the subsets of check 4 cover the frame: three strided ones exactly once, the contiguous one inside it
    strided = sorted(f + 3 * k for f in range(3) for k in range(8))
    assert strided == list(range(a["tiles"])) and 5 + 7 <= a["tiles"]

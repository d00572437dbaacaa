"""The mixed grid of pt_render_tiles: whole tiles first, the launch's last tiles as sample chunks, one launch.

A one-chunk launch without a workspace may run slots [0, n_whole) as one workgroup each and the slots from n_whole on as `chunks`
workgroups each, behind the whole ones (PtLaunch.n_whole; rt_hip_shim.hip, grid_split_for).  The shim's rule takes it only for
frames of many rounds of workgroups; RT_HIP_GRID_SPLIT=<n_whole>,<chunks> sets the split of every launch whose FORM takes one
whatever its size, which is how these tests reach the mapping at the smallest shapes where it can go wrong: one whole slot, one
chunked slot, the split in the middle, ragged tiles on either side of it, a strided subset.  Every case is compared with the
uniform one-chunk launch of the same build bit for bit -- floats as uint32, bytes, the four counters -- and
rt_hip_mixed_grid_launches() says which form a launch took, so that no comparison passes on two uniform launches.
"""
import contextlib
import os

import numpy as np
import pytest

from conftest import SEED
from util import assert_parity, fixed_point_floor, untile_numpy


@pytest.fixture(scope="module")
def gpu():
    import torch
    from rt_amd import abi, gpu as G
    assert abi.load_shim().rt_hip_device_count() >= 1, "no HIP device: the GPU tests must run on the GPU box"
    assert torch.cuda.is_available()
    return G


@contextlib.contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update({k: str(v) for k, v in kv.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _mixed_count():
    from rt_amd import abi
    return int(abi.load_shim().rt_hip_mixed_grid_launches())


def _launch(gs, first, stride, count, split=None):
    """one launch -> (float bits, bytes, counters, took the mixed form)"""
    import torch
    before = _mixed_count()
    with _env(RT_HIP_GRID_SPLIT="%d,%d" % split) if split else _env(RT_HIP_GRID_UNIFORM=1):
        t, t8, st = gs.render_tiles(SEED, first, stride, count)
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint32), t8.cpu().numpy(), st.cpu().tolist(), _mixed_count() - before == 1


def _same(got, ref, what):
    assert np.array_equal(got[0], ref[0]), f"{what}: {int((got[0] != ref[0]).any(axis=(1, 2)).sum())} tiles differ in f32"
    assert np.array_equal(got[1], ref[1]), f"{what}: bytes differ"
    assert got[2] == ref[2], f"{what}: counters {got[2]} != {ref[2]}"


@pytest.fixture(scope="module")
def frame40(gpu):
    """config 4's scene at 40 x 24 (5 x 3 = 15 whole tiles), 64 spp: the scene, and the uniform one-chunk launch, rendered once"""
    from rt_amd import scene as S
    sc = S.build_scene(4, 40, 24, 64)
    gs = gpu.GpuScene(sc)
    assert gs.kernel_name() == "pt_render_tiles"
    ref = _launch(gs, 0, 1, 15)
    assert not ref[3]
    yield sc, gs, ref
    gs.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n_whole", [1, 7, 14])
@pytest.mark.parametrize("chunks", [2, 4])
def test_split_frames_are_the_uniform_frame(gpu, frame40, n_whole, chunks):
    """one whole slot, the split in the middle, one chunked slot; 2 and 4 chunks"""
    sc, gs, ref = frame40
    got = _launch(gs, 0, 1, 15, (n_whole, chunks))
    assert got[3], "the launch did not take the mixed form"
    assert gs.last_launch_kernel() == "pt_render_tiles"
    _same(got, ref, f"n_whole {n_whole}, {chunks} chunks")


@pytest.mark.gpu
def test_the_ends_of_the_split_are_the_uniform_forms(gpu, frame40, pt):
    """n_whole = 15: the one-chunk launch itself; n_whole = 0: the uniform chunked launch, on the shim's workspace -- neither counts
    as mixed.  And the frame they all equal is the oracle's."""
    import torch
    sc, gs, ref = frame40
    for n_whole in (15, 0):
        got = _launch(gs, 0, 1, 15, (n_whole, 4))
        assert not got[3], n_whole
        _same(got, ref, f"n_whole {n_whole}")
    ws_chunked = gs.render_tiles(SEED, 0, 1, 15, chunks=4)   # the caller's own chunks and workspace: untouched by the switch
    torch.cuda.synchronize()
    _same((ws_chunked[0].cpu().numpy().view(np.uint32), ws_chunked[1].cpu().numpy(), ws_chunked[2].cpu().tolist()), ref, "chunks=4")
    got = _launch(gs, 0, 1, 15, (7, 4))
    assert got[3]
    img = untile_numpy(got[0].view(np.float32), sc.width, sc.height, 0, 1, 15, np.zeros((sc.height, sc.width, 3), dtype=np.float32))
    img8 = untile_numpy(got[1], sc.width, sc.height, 0, 1, 15, np.zeros((sc.height, sc.width, 3), dtype=np.uint8))
    mean, rgb8, ost = pt.render_pixels(sc, SEED)
    assert_parity(img, img8, dict(zip(("rays", "casts", "tests", "samples"), got[2])), mean, rgb8, ost, what="mixed 7 + 8 x 4",
                  abs_floor=fixed_point_floor(sc))
    assert got[2][3] == sc.width * sc.height * sc.samples


@pytest.mark.gpu
def test_ragged_tiles_on_either_side_of_the_split(gpu):
    """37 x 21, 16 spp: 5 x 3 tiles, the right column 5 wide (slots 4, 9, 14), the bottom row 5 high (slots 10 .. 14).  n_whole = 7:
    ragged slot 4 is whole, ragged slots 9 .. 14 are chunked; n_whole = 12: the bottom row's slots 10, 11 are whole as well.  Three
    chunks of 16 samples: 5 + 5 + 6."""
    from rt_amd import scene as S
    sc = S.build_scene(4, 37, 21, 16)
    gs = gpu.GpuScene(sc)
    ref = _launch(gs, 0, 1, 15)
    for split in ((7, 3), (12, 2), (4, 16)):
        got = _launch(gs, 0, 1, 15, split)
        assert got[3], split
        _same(got, ref, f"37 x 21, split {split}")
    gs.close()


@pytest.mark.gpu
def test_a_strided_subset_with_the_split_inside(gpu, frame40):
    """tiles 1, 4, 7, 10, 13 (first 1, stride 3, count 5), whole slots 0 .. 1, chunked slots 2 .. 4: the slot, not the tile, decides,
    and every output and workspace address follows from the slot"""
    sc, gs, whole = frame40
    ref = _launch(gs, 1, 3, 5)
    assert np.array_equal(ref[0], whole[0][1::3]), "the subset's uniform launch is not the whole frame's tiles"
    for split in ((2, 4), (1, 2), (4, 3)):
        got = _launch(gs, 1, 3, 5, split)
        assert got[3], split
        _same(got, ref, f"subset, split {split}")


@pytest.mark.gpu
def test_forms_that_do_not_take_the_mixed_plan_are_left_alone(gpu):
    """with the switch set: a pass of an accumulation (sums that outlive the launch), a room with M_CHECKERED (another member), a
    caller's own chunks -- none is mixed, each renders what it rendered"""
    import torch
    from rt_amd import scene as S
    from util import class_scene
    sc = S.build_scene(4, 40, 24, 64)
    gs = gpu.GpuScene(sc)
    ref = _launch(gs, 0, 1, 15)
    before = _mixed_count()
    with _env(RT_HIP_GRID_SPLIT="7,4"):
        acc = gs.accumulate(SEED, 64)
        st = torch.zeros(4, dtype=torch.int64, device="cuda")
        acc.add(64, stats=st)
        t, t8 = acc.resolve()
        torch.cuda.synchronize()
        assert acc.kernel == "pt_render_tiles"
        _same((t.cpu().numpy().view(np.uint32), t8.cpu().numpy(), st.cpu().tolist()), ref, "one pass of 64")
        acc.close()
        t, t8, st = gs.render_tiles(SEED, 0, 1, 15, chunks=2)
        torch.cuda.synchronize()
        _same((t.cpu().numpy().view(np.uint32), t8.cpu().numpy(), st.cpu().tolist()), ref, "the caller's chunks")
    gs.close()
    chk = class_scene(n_packed=4, chk=True)
    chk.width, chk.height, chk.samples = 40, 24, 16
    gc = gpu.GpuScene(chk)
    assert gc.kernel_name() == "pt_render_tiles_chk"
    ref = _launch(gc, 0, 1, 15)
    got = _launch(gc, 0, 1, 15, (7, 4))
    _same(got, ref, "M_CHECKERED room")
    gc.close()
    chk.free()
    assert _mixed_count() == before


@pytest.mark.gpu
def test_without_its_workspace_the_launch_is_uniform(gpu, frame40):
    """the workspace's allocation made to fail: the same bits through the uniform form, and the mixed form again afterwards"""
    from rt_amd import abi
    sc, gs, ref = frame40
    shim = abi.load_shim()
    shim.rt_hip_release_cache()   # no workspace yet: the launch has to ask for one
    shim.rt_hip_selftest_fail_alloc(abi.FAIL_ALLOC_TAIL_WS)
    try:
        got = _launch(gs, 0, 1, 15, (7, 4))
    finally:
        shim.rt_hip_selftest_fail_alloc(0)
    assert not got[3]
    _same(got, ref, "no workspace")
    got = _launch(gs, 0, 1, 15, (7, 4))
    assert got[3]
    _same(got, ref, "workspace back")


@pytest.mark.gpu
def test_the_rule_leaves_small_launches_as_they_are(gpu, frame40):
    """no switch set: 15 tiles are far below the rounds of workgroups the rule asks for"""
    import torch
    sc, gs, ref = frame40
    before = _mixed_count()
    t, t8, st = gs.render_tiles(SEED, 0, 1, 15)
    torch.cuda.synchronize()
    assert _mixed_count() == before
    _same((t.cpu().numpy().view(np.uint32), t8.cpu().numpy(), st.cpu().tolist()), ref, "no switch")


@pytest.mark.gpu
def test_the_rule_takes_a_frame_of_many_rounds_by_itself(gpu):
    """no switch set: 1920 x 1080 (32,400 tiles: more than 8 rounds of the workgroups any device of this family holds) at 512 spp,
    the rule's sample floor (4 chunks x 128), takes the mixed form by itself and renders the uniform launch's bits; one sample
    fewer and the launch stays uniform.  (~0.1 s a launch.)"""
    import torch
    from rt_amd import scene as S
    sc = S.build_scene(4, 1920, 1080, 512)
    gs = gpu.GpuScene(sc)
    assert gs.kernel_name() == "pt_render_tiles"
    tiles = gpu.n_tiles(sc.width, sc.height)
    ref = _launch(gs, 0, 1, tiles)
    assert not ref[3]
    before = _mixed_count()
    t, t8, st = gs.render_tiles(SEED, 0, 1, tiles)
    torch.cuda.synchronize()
    assert _mixed_count() - before == 1, "the rule did not take the mixed form at 32,400 tiles, 512 spp"
    _same((t.cpu().numpy().view(np.uint32), t8.cpu().numpy(), st.cpu().tolist()), ref, "the rule's own split")
    gs.close()
    sc = S.build_scene(4, 1920, 1080, 511)
    gs = gpu.GpuScene(sc)
    before = _mixed_count()
    gs.render_tiles(SEED, 0, 1, tiles)
    torch.cuda.synchronize()
    assert _mixed_count() == before, "511 spp: under the floor of 128 samples a chunk"
    gs.close()

"""The retry stack of the pooled kernels' direction rounds (pt_body_pooled.h, PT_DIR_PARK).

A lane of a swapping pooled kernel whose diffuse hit still lacks its direction sample after the trip's rounds writes its path
to the top of the wave's 64-entry waiting list and goes idle; lanes that are idle just before a later trip's rounds take such
paths back.  Which lane draws a sample, and in which trip, must not show anywhere: frames, bytes, rays and ray-bounces meet the
oracle's under the suite's parity helper (util.assert_parity: counters equal, floats to 1e-6 relative, bytes to one step), and
are bit for bit the same between GPU runs, whatever the partition into tiles, sample chunks and passes, and in the build that
carries retries in their lane (-DPT_DIR_PARK=0).

Shapes: the smallest launches that reach each path of the block.  One full tile at 16 spp is 1,024 jobs for four waves: every
wave swaps (more than 64 jobs), parks, and drains its stack at the pool's end.  13 x 9 has ragged tiles (5 and 1 pixels wide or
high: batches that are no sample index of a whole tile).  The all-diffuse room fills the list from both ends, so that retries
find no room and are carried as before the stack existed (asserted through the PT_DIAG build's counter, in a child process)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import SEED
from util import assert_parity, fixed_point_floor, tile_pixels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raytracer.c_amd", "csrc")
DIAG_LIB = os.path.join(CSRC, "librt_hip_diag.so")


from dir_park_scenes import (DEEP_GLASS_DEPTH, KERNELS, PARK_ROWS, PARK_SCENES, REFR_SCENES, SCENES, deep_glass_room, diffuse_room,
                             room_ragged, room_tile)


@pytest.fixture(scope="module")
def gpu():
    import torch
    from rt_amd import abi, gpu as G
    assert abi.load_shim().rt_hip_device_count() >= 1, "no HIP device: the GPU tests must run on the GPU box"
    assert torch.cuda.is_available()
    return G


_ORACLE = {}


def _oracle(pt, name, sc, pixels=None):
    """the oracle's frame of a scene, computed once per (scene, pixel set) and left unchanged"""
    key = (name, None if pixels is None else tuple(pixels.tolist()))
    if key not in _ORACLE:
        mean, rgb8, st = pt.render_pixels(sc, SEED, pixels=pixels)
        assert np.isfinite(mean).all(), f"{name}: the oracle's own frame is not finite"
        mean.setflags(write=False)
        rgb8.setflags(write=False)
        _ORACLE[key] = (mean, rgb8, st)
    return _ORACLE[key]


def _tiles(gs, first, stride, count, chunks=1):
    import torch
    t, t8, st = gs.render_tiles(SEED, first, stride, count, chunks=chunks)
    torch.cuda.synchronize()
    return t.cpu().numpy(), t8.cpu().numpy(), dict(zip(("rays", "casts", "tests", "samples"), st.cpu().tolist()))


def _inside(sc, t, t8, ids):
    """the inside-image pixels of rendered tiles `ids`, in util.tile_pixels' order"""
    tx = (sc.width + 7) // 8
    f, b = [], []
    for k, tile in enumerate(ids):
        x0, y0 = (tile % tx) * 8, (tile // tx) * 8
        for r in range(8):
            for c in range(8):
                if x0 + c < sc.width and y0 + r < sc.height:
                    f.append(t[k, r * 8 + c])
                    b.append(t8[k, r * 8 + c])
    return np.array(f), np.array(b)


def _same(a, b, what):
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)), f"{what}: frame floats differ"
    assert np.array_equal(a[1], b[1]), f"{what}: frame bytes differ"


@pytest.mark.gpu
def test_one_full_tile_is_the_oracle_s_in_one_chunk_and_in_three(gpu, pt):
    sc = room_tile()
    gs = gpu.GpuScene(sc)
    one = _tiles(gs, 0, 1, 1)
    assert gs.last_launch_kernel() == "pt_render_tiles"
    three = _tiles(gs, 0, 1, 1, chunks=3)
    assert gs.last_launch_kernel() == "pt_render_tiles"
    gs.launch_status()
    gs.close()
    px = tile_pixels(sc.width, sc.height, [0])
    mean, rgb8, ost = _oracle(pt, "room_tile", sc, px)
    assert_parity(one[0][0], one[1][0], one[2], mean, rgb8, ost, what="one tile", abs_floor=fixed_point_floor(sc))
    _same(one, three, "3 sample chunks")
    assert one[2] == three[2], (one[2], three[2])
    sc.free()


@pytest.mark.gpu
def test_ragged_tiles_whole_and_strided_agree_with_each_other_and_the_oracle(gpu, pt):
    sc = room_ragged()
    total = gpu.n_tiles(sc.width, sc.height)
    assert total == 4
    gs = gpu.GpuScene(sc)
    whole = _tiles(gs, 0, 1, total)
    assert gs.last_launch_kernel() == "pt_render_tiles"
    odd = _tiles(gs, 1, 2, 2)
    gs.launch_status()
    gs.close()
    ids = list(range(total))
    f, b = _inside(sc, whole[0], whole[1], ids)
    mean, rgb8, ost = _oracle(pt, "room_ragged", sc, tile_pixels(sc.width, sc.height, ids))
    assert_parity(f, b, whole[2], mean, rgb8, ost, what="13 x 9 whole", abs_floor=fixed_point_floor(sc))
    _same((whole[0][[1, 3]], whole[1][[1, 3]]), (odd[0][:2], odd[1][:2]), "tiles 1, 3 alone")
    f, b = _inside(sc, odd[0], odd[1], [1, 3])
    mean, rgb8, ost = _oracle(pt, "room_ragged", sc, tile_pixels(sc.width, sc.height, [1, 3]))
    assert_parity(f, b, odd[2], mean, rgb8, ost, what="13 x 9 tiles 1, 3", abs_floor=fixed_point_floor(sc))
    sc.free()


def _child(lib, scene, chunks=1):
    """one child process renders `scene` (a comma-separated list: one record per scene, in a list) with the build `lib`"""
    assert os.path.exists(lib), lib
    env = dict(os.environ, RT_HIP_SHIM_PATH=lib)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "dir_park_child.py"), scene, str(chunks)], env=env,
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    recs = [json.loads(ln) for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(recs) == len(scene.split(",")), p.stdout[-2000:]
    return recs[0] if len(recs) == 1 else recs


@pytest.mark.gpu
def test_all_diffuse_room_fills_the_list_and_retries_without_room_are_carried(gpu, pt):
    sc = diffuse_room()
    gs = gpu.GpuScene(sc)
    got = _tiles(gs, 0, 1, 1)
    assert gs.last_launch_kernel() == "pt_render_tiles"
    gs.launch_status()
    gs.close()
    mean, rgb8, ost = _oracle(pt, "diffuse_room", sc, tile_pixels(sc.width, sc.height, [0]))
    # the scene is what it is meant to be: paths end at the depth limit, a direction per bounce (5.2 bounces a path on the headline scene)
    assert ost["rays"] > 15 * sc.width * sc.height * sc.samples, ost   # nearly every path lives to the depth limit
    assert_parity(got[0][0], got[1][0], got[2], mean, rgb8, ost, what="all-diffuse room", abs_floor=fixed_point_floor(sc))
    # the PT_DIAG build of the same kernel, in a child process: paths were parked, some found no room, and its frame is this one
    rec = _child(DIAG_LIB, "diffuse_room")
    print("all-diffuse room, PT_DIAG:", rec)
    assert rec["kernel"] == "pt_render_tiles" and rec["violations"] == 0
    assert rec["stats"][:2] == [got[2]["rays"], got[2]["casts"]], rec
    assert rec["parked"] > 0, rec
    assert rec["no_room"] > 0, rec
    sc.free()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["config2", "config3", "checkered", "glass"])
def test_the_other_swapping_kernels_render_the_oracle_s_frame(gpu, pt, name):
    sc = SCENES[name]()
    total = gpu.n_tiles(sc.width, sc.height)
    gs = gpu.GpuScene(sc)
    got = _tiles(gs, 0, 1, total)
    assert gs.last_launch_kernel() == KERNELS[name], gs.last_launch_kernel()
    split = _tiles(gs, 0, 1, total, chunks=2)
    assert gs.last_launch_kernel() == KERNELS[name], gs.last_launch_kernel()
    gs.launch_status()
    gs.close()
    ids = list(range(total))
    f, b = _inside(sc, got[0], got[1], ids)
    mean, rgb8, ost = _oracle(pt, name, sc, tile_pixels(sc.width, sc.height, ids))
    assert_parity(f, b, got[2], mean, rgb8, ost, what=name, hdr=True, abs_floor=fixed_point_floor(sc))
    _same(got, split, f"{name}: 2 sample chunks")
    assert got[2] == split[2]
    sc.free()


@pytest.mark.gpu
def test_two_passes_end_at_the_one_shot_frame(gpu):
    import torch
    sc = room_tile()
    gs = gpu.GpuScene(sc)
    t, t8, st = gs.render_tiles(SEED, 0, 1, 1, chunks=gs.suggest_chunks(1))
    torch.cuda.synchronize()
    one = (t.cpu().numpy(), t8.cpu().numpy())
    acc = gs.accumulate(SEED, sc.samples)
    stats = torch.zeros(4, dtype=torch.int64, device=torch.device("cuda", gs.device))
    for n in (5, 11):
        acc.add(n, stats)
    at, at8 = acc.resolve()
    torch.cuda.synchronize()
    assert acc.kernel == "pt_render_tiles" and acc.samples == sc.samples
    _same(one, (at.cpu().numpy(), at8.cpu().numpy()), "passes of 5 + 11 samples")
    assert stats.tolist() == st.tolist(), (stats.tolist(), st.tolist())
    gs.launch_status()
    acc.close()
    gs.close()
    sc.free()


PARK0_LIB = os.path.join(CSRC, "variants", "librt_hip_park0.so")


@pytest.mark.gpu
def test_park_and_carry_builds_give_the_same_frame(gpu):
    """the A/B knob's other arm (-DPT_DIR_PARK=0: retries carried in their lane, four rounds; `make all` builds it next to the
    shipped library) against the shipped build, on the first case, each in a child process: the same kernel, identical frame
    floats, frame bytes and counters"""
    assert os.path.exists(PARK0_LIB), f"{PARK0_LIB} missing: run `make` at the repository root (target shim-park0)"
    shipped = os.path.join(CSRC, "librt_hip.so")
    carry, park = _child(PARK0_LIB, "room_tile"), _child(shipped, "room_tile")
    assert carry["kernel"] == park["kernel"] == "pt_render_tiles", (carry, park)
    for key in ("frame", "frame8", "stats"):
        assert carry[key] == park[key], (key, carry, park)


# ---- the retry stack in every swapping kernel --------------------------------------------------------------------------------
# One all-diffuse, closed, deep-path room per kernel (dir_park_scenes.PARK_ROWS; tests/test_dir_park_scenes_cpu.py shows on the
# CPU that they are that): one 8 x 8 tile at 64 spp and depth 16 is 4,096 jobs for four waves, so every wave swaps with live
# paths on its list, its stack grows until it meets the list from above, and the pool's end is drained from the stack.  Three
# child processes render all of them: the PT_DIAG build, the carrying build and the shipped library.
SHIPPED_LIB = os.path.join(CSRC, "librt_hip.so")
CHILD_LIST = ",".join(PARK_SCENES + ["deep_glass:0"])
_BUILDS = {}


def _build_records(lib):
    """scene -> the child's record, every scene of CHILD_LIST rendered by one child process per build"""
    if lib not in _BUILDS:
        _BUILDS[lib] = {r["scene"]: r for r in _child(lib, CHILD_LIST)}
        if lib == DIAG_LIB:
            for r in _BUILDS[lib].values():
                print("PT_DIAG:", r)
    return _BUILDS[lib]


@pytest.mark.gpu
@pytest.mark.parametrize("name,kernel", [(r[0], r[1]) for r in PARK_ROWS], ids=[r[1] for r in PARK_ROWS])
def test_every_swapping_kernel_s_room_is_the_oracle_s_in_one_chunk_and_in_three(gpu, pt, name, kernel):
    sc = SCENES[name]()
    assert (sc.width, sc.height, sc.samples, sc.max_depth) == (8, 8, 64, 16)
    gs = gpu.GpuScene(sc)
    one = _tiles(gs, 0, 1, 1)
    assert gs.last_launch_kernel() == kernel == KERNELS[name], gs.last_launch_kernel()
    three = _tiles(gs, 0, 1, 1, chunks=3)
    assert gs.last_launch_kernel() == kernel, gs.last_launch_kernel()
    gs.launch_status()
    gs.close()
    mean, rgb8, ost = _oracle(pt, name, sc, tile_pixels(sc.width, sc.height, [0]))
    print(name, kernel, "gpu", one[2], "oracle", ost, "worst relative error",
          float((np.abs(one[0][0].astype(np.float64) - mean) / np.maximum(np.abs(mean), 1e-300)).max()))
    assert_parity(one[0][0], one[1][0], one[2], mean, rgb8, ost, what=name, hdr=True, abs_floor=fixed_point_floor(sc))
    _same(one, three, f"{name}: 3 sample chunks")
    assert one[2] == three[2], (one[2], three[2])
    sc.free()


@pytest.mark.gpu
@pytest.mark.parametrize("name,kernel", [(r[0], r[1]) for r in PARK_ROWS], ids=[r[1] for r in PARK_ROWS])
def test_carrying_and_diag_builds_render_the_shipped_build_s_room(gpu, name, kernel):
    """-DPT_DIR_PARK=0 (retries carried in their lane) gives the shipped build's frame digest, byte digest and counters; the
    PT_DIAG build its rays and casts, with no violation of a conservative rule"""
    assert os.path.exists(PARK0_LIB), f"{PARK0_LIB} missing: run `make` at the repository root (target shim-park0)"
    park, carry, diag = (_build_records(lib)[name] for lib in (SHIPPED_LIB, PARK0_LIB, DIAG_LIB))
    assert park["kernel"] == carry["kernel"] == diag["kernel"] == kernel, (park, carry, diag)
    for key in ("frame", "frame8", "stats"):
        assert carry[key] == park[key], (key, carry, park)
    assert diag["stats"][:2] == park["stats"][:2], (diag, park)
    assert diag["violations"] == 0, diag


@pytest.mark.gpu
@pytest.mark.parametrize("name,kernel", [(r[0], r[1]) for r in PARK_ROWS], ids=[r[1] for r in PARK_ROWS])
def test_every_room_drives_its_kernel_s_retry_stack_to_collision(gpu, name, kernel):
    """conditions on the inputs, not measurements: the PT_DIAG build's counters of the rooms (profiles/r11_dir_park_reach.txt)"""
    rec = _build_records(DIAG_LIB)[name]
    assert rec["kernel"] == kernel, rec
    assert rec["parked"] > 0, rec
    if name in REFR_SCENES:
        assert rec["parked_children"] > 0, rec
    else:
        assert rec["parked_children"] == 0, rec
        assert rec["no_room"] > 0, rec
        assert rec["swaps_put_off"] > 0, rec
        assert rec["dry_drains"] > 0, rec


@pytest.mark.gpu
def test_some_refraction_room_fills_the_list_and_puts_swaps_off(gpu):
    recs = [_build_records(DIAG_LIB)[n] for n in REFR_SCENES]
    assert len(recs) == 3
    assert any(r["no_room"] > 0 for r in recs), recs
    assert any(r["swaps_put_off"] > 0 for r in recs), recs


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["passes_refr", "passes_mem_s"])
def test_two_passes_end_at_the_one_shot_frame_in_two_further_kernels(gpu, name):
    """5 + 11 samples against the 16-spp one-shot frame; the M_REFRACTION form takes the epilogue's acc_keep branch with
    windowed sums there"""
    import torch
    sc = SCENES[name]()
    assert sc.samples == 16
    gs = gpu.GpuScene(sc)
    t, t8, st = gs.render_tiles(SEED, 0, 1, 1, chunks=gs.suggest_chunks(1))
    torch.cuda.synchronize()
    assert gs.last_launch_kernel() == KERNELS[name], gs.last_launch_kernel()
    one = (t.cpu().numpy(), t8.cpu().numpy())
    acc = gs.accumulate(SEED, sc.samples)
    stats = torch.zeros(4, dtype=torch.int64, device=torch.device("cuda", gs.device))
    for n in (5, 11):
        acc.add(n, stats)
    at, at8 = acc.resolve()
    torch.cuda.synchronize()
    assert acc.kernel == KERNELS[name] and acc.samples == sc.samples
    _same(one, (at.cpu().numpy(), at8.cpu().numpy()), f"{name}: passes of 5 + 11 samples")
    assert stats.tolist() == st.tolist(), (stats.tolist(), st.tolist())
    gs.launch_status()
    acc.close()
    gs.close()
    sc.free()


@pytest.mark.gpu
def test_the_refraction_entry_s_depth_field_past_bit_3(gpu, pt):
    """the glass room at 32 spp and max_depth 26 (DEEP_GLASS_DEPTH): the largest depth <= 28 at which the shim's own chunk
    count leaves a chunk 8 samples (two batches a wave) and the launch stays on pt_render_tiles_refr_pool; the entry's 6-bit
    depth field then carries values past 15"""
    sc = deep_glass_room()
    assert sc.samples == 32 and 16 < sc.max_depth == DEEP_GLASS_DEPTH <= 28
    gs = gpu.GpuScene(sc)
    for deeper in range(28, DEEP_GLASS_DEPTH, -1):   # the shim's answers: deeper, a chunk keeps fewer than 8 samples
        assert 32 // gs.suggest_chunks(1, samples=32, max_depth=deeper) < 8, deeper
    chunks = gs.suggest_chunks(1, samples=32, max_depth=sc.max_depth)
    assert chunks > 1 and 32 // chunks >= 8, chunks
    got = _tiles(gs, 0, 1, 1, chunks=chunks)
    assert gs.last_launch_kernel() == "pt_render_tiles_refr_pool", gs.last_launch_kernel()
    gs.launch_status()
    gs.close()
    mean, rgb8, ost = _oracle(pt, "deep_glass", sc, tile_pixels(sc.width, sc.height, [0]))
    assert_parity(got[0][0], got[1][0], got[2], mean, rgb8, ost, what="deep glass room", hdr=True, abs_floor=fixed_point_floor(sc))
    rec = _build_records(DIAG_LIB)["deep_glass"]
    assert rec["kernel"] == "pt_render_tiles_refr_pool" and rec["chunks"] == chunks and rec["violations"] == 0, rec
    assert rec["stats"][:2] == [got[2]["rays"], got[2]["casts"]], (rec, got[2])
    assert rec["parked_children"] > 0, rec
    sc.free()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ragged_chk", "ragged_refr"])
def test_ragged_tiles_of_a_checkered_and_a_glass_room(gpu, pt, name):
    sc = SCENES[name]()
    total = gpu.n_tiles(sc.width, sc.height)
    assert (sc.width, sc.height, total) == (13, 9, 4)
    gs = gpu.GpuScene(sc)
    whole = _tiles(gs, 0, 1, total)
    assert gs.last_launch_kernel() == KERNELS[name], gs.last_launch_kernel()
    odd = _tiles(gs, 1, 2, 2)
    assert gs.last_launch_kernel() == KERNELS[name], gs.last_launch_kernel()
    gs.launch_status()
    gs.close()
    ids = list(range(total))
    f, b = _inside(sc, whole[0], whole[1], ids)
    mean, rgb8, ost = _oracle(pt, name, sc, tile_pixels(sc.width, sc.height, ids))
    assert_parity(f, b, whole[2], mean, rgb8, ost, what=f"{name} 13 x 9 whole", hdr=True, abs_floor=fixed_point_floor(sc))
    _same((whole[0][[1, 3]], whole[1][[1, 3]]), (odd[0][:2], odd[1][:2]), f"{name}: tiles 1, 3 alone")
    sc.free()

"""The mixed grid of pt_render_tiles where its addressing and ordering are tightest (tests/test_gpu_mixed_grid.py holds the mapping
itself, on config 4's room): NaN masks on both sides of every split, sums at the edges of the fixed-point range, the smallest
grids, the shim's workspace grown, released and handed between streams, the rule without a switch at its threshold in tiles and
over a strided share, a launch without its optional outputs, and rt_hip_render_image, the C hosts' form.

The reference of every case is the uniform one-chunk launch of the same build (RT_HIP_GRID_UNIFORM=1), compared bit for bit: floats
as uint32 (a NaN equals a NaN of the same bits), the byte tiles, the four counters.  That is the contract the feature states, so
there is no tolerance anywhere; the uniform form itself is held to the oracle by test_gpu_parity, test_gpu_sum_range and
test_gpu_edges on the same scenes.  rt_hip_mixed_grid_launches() says which form every launch took.
"""
import ctypes as C

import numpy as np
import pytest

from conftest import SEED
from test_gpu_mixed_grid import _env, _launch, _mixed_count, _same

pytestmark = pytest.mark.gpu

MIN_ROUNDS = 8      # rt_hip_shim.hip, GRID_TAIL_MIN_ROUNDS: the rule asks for this many rounds of resident workgroups
HD = (1920, 1080, 512)
_CACHE = {}         # name -> what a scene's builder returned; closed by the module's last test


@pytest.fixture(scope="module")
def gpu():
    import torch
    from rt_amd import abi, gpu as G
    assert abi.load_shim().rt_hip_device_count() >= 1, "no HIP device: the GPU tests must run on the GPU box"
    assert torch.cuda.is_available()
    return G


def _cached(name, make):
    if name not in _CACHE:
        _CACHE[name] = make()
    return _CACHE[name]


def _room(gpu, width, height, samples):
    """config 4's room at a size: (scene, GpuScene, tiles, the uniform one-chunk launch), rendered once"""
    def make():
        from rt_amd import scene as S
        sc = S.build_scene(4, width, height, samples)
        gs = gpu.GpuScene(sc)
        assert gs.kernel_name() == "pt_render_tiles"
        tiles = gpu.n_tiles(width, height)
        ref = _launch(gs, 0, 1, tiles)
        assert not ref[3]
        return sc, gs, tiles, ref
    return _cached(("room", width, height, samples), make)


def _custom_frame(gpu, name, make_scene):
    """a scene of accum_range_scenes: (scene, GpuScene, tiles, the uniform one-chunk launch); pt_render_tiles or the row is wrong"""
    def make():
        sc = make_scene()
        gs = gpu.GpuScene(sc)
        assert gs.kernel_name() == "pt_render_tiles", f"{name}: {gs.kernel_name()} takes no mixed grid"
        tiles = gpu.n_tiles(sc.width, sc.height)
        ref = _launch(gs, 0, 1, tiles)
        assert not ref[3] and gs.last_launch_kernel() == "pt_render_tiles"
        return sc, gs, tiles, ref
    return _cached(name, make)


def _split_is_the_uniform_frame(gs, ref, first, stride, count, split, what):
    got = _launch(gs, first, stride, count, split)
    assert got[3], f"{what}, split {split}: the launch did not take the mixed form"
    _same(got, ref, f"{what}, split {split}")
    return got


# ---- 1. NaN samples on both sides of every split --------------------------------------------------------------------------------
NAN_W, NAN_H, NAN_SPP, NAN_TILES = 24, 16, 9, 6


def _nan_frame(gpu):
    import accum_range_scenes as A
    return _custom_frame(gpu, "nan", lambda: A.nan_scene(None, NAN_SPP))


def _nan_tiles(frame):
    """the slots of a launch that hold a NaN pixel"""
    return [k for k in range(frame[0].shape[0]) if np.isnan(frame[0][k].view(np.float32)).any()]


def _nan_frame_checks(got, what):
    nan = np.isnan(got[0].view(np.float32))
    assert (got[1][nan] == 255).all(), f"{what}: a NaN pixel's byte is not 255"


def test_nan_scene_has_nan_tiles_and_finite_ones(gpu):
    """the premise of the NaN cases: the uniform frame has NaN and finite pixels, NaN pixels in two tiles at least, and the 30
    splits below put a NaN-holding tile on the whole side (n_whole = 5 leaves only tile 5 chunked) and on the chunked side
    (n_whole = 1 leaves only tile 0 whole) at least once each"""
    sc, gs, tiles, ref = _nan_frame(gpu)
    assert (sc.width, sc.height, sc.samples, tiles) == (NAN_W, NAN_H, NAN_SPP, NAN_TILES)
    f = ref[0].view(np.float32)
    assert np.isnan(f).any() and np.isfinite(f[f != 0]).any(), "the scene renders no NaN pixel, or nothing else"
    held = _nan_tiles(ref)
    print(f"NaN-holding tiles of the {NAN_W} x {NAN_H} frame: {held}")
    assert len(held) >= 2
    whole_side = {t for n_whole in range(1, NAN_TILES) for t in held if t < n_whole}
    chunked_side = {t for n_whole in range(1, NAN_TILES) for t in held if t >= n_whole}
    assert whole_side and chunked_side, (held, whole_side, chunked_side)
    _nan_frame_checks(ref, "uniform")
    assert ref[2][3] == NAN_W * NAN_H * NAN_SPP


@pytest.mark.parametrize("chunks", [2, 3, 9])
@pytest.mark.parametrize("n_whole", [1, 2, 3, 4, 5])
def test_nan_masks_on_both_sides_of_the_split(gpu, n_whole, chunks):
    """a chunked slot ORs its masks in behind the chunked slots' records, at record slot - n_whole, and the resolve reads them
    there; a whole slot never touches the workspace"""
    sc, gs, tiles, ref = _nan_frame(gpu)
    got = _split_is_the_uniform_frame(gs, ref, 0, 1, tiles, (n_whole, chunks), "NaN frame")
    _nan_frame_checks(got, f"split ({n_whole}, {chunks})")
    assert got[2][3] == NAN_W * NAN_H * NAN_SPP


def test_nan_masks_over_a_strided_subset(gpu):
    """tiles 1, 3, 5 (first 1, stride 2, count 3) -- or 0, 2, 4 where none of those holds a NaN: the two subsets cover the frame
    -- with one and with two whole slots: the masks follow the slot, not the tile"""
    sc, gs, tiles, whole = _nan_frame(gpu)
    held = _nan_tiles(whole)
    first = 1 if any(t % 2 == 1 for t in held) else 0
    ref = _launch(gs, first, 2, 3)
    assert not ref[3] and np.array_equal(ref[0], whole[0][first::2]), "the subset's uniform launch is not the frame's tiles"
    in_subset = _nan_tiles(ref)
    print(f"NaN-holding slots of the subset first {first}, stride 2: {in_subset}")
    assert in_subset, "the subset holds no NaN tile"
    for split in ((1, 2), (2, 3)):
        got = _split_is_the_uniform_frame(gs, ref, first, 2, 3, split, f"NaN subset from {first}")
        _nan_frame_checks(got, f"subset, split {split}")
        assert got[2][3] == ref[2][3]


# ---- 2. the edges of the fixed-point range --------------------------------------------------------------------------------------
RANGE_SPP = 16


def _brightest_fixed_point_emitter():
    """the brightest hidden emitter whose 40 x 24, 16-spp launch keeps fixed-point sums, i.e. stays with pt_render_tiles: the rule
    tests/test_gpu_sum_range.py picks its kernels by (accum_range_scenes._fixed_point_fits, pt_fixed_sums_fit restated), bisected
    between that file's 1e3, which fits, and its 1e6, which does not; a millionth below the edge, away from the rounding of the
    restatement"""
    import types
    import accum_range_scenes as A
    probe = types.SimpleNamespace(max_depth=5, samples=RANGE_SPP)   # all the rule reads of a scene
    lo, hi = 1e3, 1e6
    assert A._fixed_point_fits(probe, lo) and not A._fixed_point_fits(probe, hi)
    for _ in range(60):
        mid = (lo * hi) ** 0.5
        lo, hi = (mid, hi) if A._fixed_point_fits(probe, mid) else (lo, mid)
    return lo * (1.0 - 1e-6)


def _range_rows():
    import accum_range_scenes as A
    return {"negative sums": lambda: A.negative_emission_scene(samples=RANGE_SPP),
            "coarse scale": lambda: A.hidden_emitter_scene(1e3, samples=RANGE_SPP),
            "brightest fixed point": lambda: A.hidden_emitter_scene(_brightest_fixed_point_emitter(), samples=RANGE_SPP)}


@pytest.mark.parametrize("row", ["negative sums", "coarse scale", "brightest fixed point"])
def test_range_edges_on_both_sides_of_the_split(gpu, row):
    """whole slots finish in the kernel, chunked slots in pt_resolve_tiles: both with the launch's scale and sample count, over
    negative two's-complement sums, a coarse scale and the coarsest scale the member accepts.  One whole slot, the middle, one
    chunked slot; chunks of 8 samples and of 1"""
    sc, gs, tiles, ref = _custom_frame(gpu, row, _range_rows()[row])
    assert (sc.width, sc.height, sc.samples, tiles) == (40, 24, RANGE_SPP, 15)
    if row == "negative sums":
        assert (ref[0].view(np.float32) < 0).any(), "no negative pixel: the sums are not negative anywhere"
    if row == "brightest fixed point":
        import accum_range_scenes as A
        print(f"brightest emitter with fixed-point sums at {RANGE_SPP} spp: {A.max_emission(sc):.6g}")
        assert A.max_emission(sc) > 1e4
    for chunks in (2, RANGE_SPP):
        for n_whole in (1, 7, 14):
            _split_is_the_uniform_frame(gs, ref, 0, 1, tiles, (n_whole, chunks), row)
    assert gs.last_launch_kernel() == "pt_render_tiles"


# ---- 3. the smallest grids ------------------------------------------------------------------------------------------------------
SMALLEST = [
    (16, 8, 2, (1, 2)),   # 2 tiles, one whole and one chunked; samples == chunks == 2
    (16, 8, 3, (1, 3)),   # samples == chunks
    (16, 8, 3, (1, 2)),   # chunks of 1 + 2 samples
    (9, 9, 4, (1, 2)),    # 4 tiles, three of them ragged, the last 1 x 1 pixel: ragged tiles chunked
    (9, 9, 4, (3, 2)),    # ... and whole, the 1 x 1 tile alone chunked
]


@pytest.mark.parametrize("width,height,samples,split", SMALLEST, ids=[f"{w}x{h}-{s}spp-{a}+{b}" for w, h, s, (a, b) in SMALLEST])
def test_smallest_grids(gpu, width, height, samples, split):
    sc, gs, tiles, ref = _room(gpu, width, height, samples)
    assert tiles == (2 if width == 16 else 4)
    _split_is_the_uniform_frame(gs, ref, 0, 1, tiles, split, f"{width} x {height}, {samples} spp")


def test_documented_ends_of_the_switch(gpu):
    """RT_HIP_GRID_SPLIT, as rt_hip_shim.hip states it: n_whole >= the slots, chunks < 2 and chunks > samples leave the uniform
    one-chunk launch; n_whole = 0 is the uniform chunked launch on the shim's workspace.  None counts as mixed, each renders the
    uniform frame -- on 15 tiles at 64 spp and on the two-tile grid at 3 spp"""
    for (width, height, samples), switches in (((40, 24, 64), ((15, 4), (16, 4), (1000, 2), (7, 1), (7, 0), (7, 65), (0, 4), (0, 64))),
                                               ((16, 8, 3), ((2, 2), (1, 1), (1, 4), (0, 2), (0, 3)))):
        sc, gs, tiles, ref = _room(gpu, width, height, samples)
        for switch in switches:
            got = _launch(gs, 0, 1, tiles, switch)
            assert not got[3], f"{width} x {height}: RT_HIP_GRID_SPLIT={switch} counted as mixed"
            _same(got, ref, f"{width} x {height}, RT_HIP_GRID_SPLIT={switch}")


# ---- 4. the workspace grows, is released, and is handed between streams ---------------------------------------------------------
def test_workspace_grows_and_is_released(gpu):
    """released; one chunked slot (the smallest workspace); 14 chunked slots (held and too small: the device drains, the
    workspace is freed and allocated again); one chunked slot on the larger workspace; the rule's own 1,080p launch (a round of
    resident workgroups' worth of slots: it grows again); one chunked slot once more; released with nothing in flight, and the
    next split allocates again.  Every frame is its uniform frame, every launch counts as mixed"""
    from rt_amd import abi
    shim = abi.load_shim()
    sc, gs, tiles, ref = _room(gpu, 40, 24, 64)
    hsc, hgs, htiles, href = _room(gpu, *HD)
    shim.rt_hip_release_cache()
    for split in ((14, 4), (1, 4), (14, 4)):
        _split_is_the_uniform_frame(gs, ref, 0, 1, tiles, split, "15 tiles, the workspace growing")
    import torch
    before = _mixed_count()
    t, t8, st = hgs.render_tiles(SEED, 0, 1, htiles)
    torch.cuda.synchronize()
    assert _mixed_count() - before == 1, "the rule did not take the mixed form at 1,080p, 512 spp"
    _same((t.cpu().numpy().view(np.uint32), t8.cpu().numpy(), st.cpu().tolist()), href, "1,080p on the grown workspace")
    _split_is_the_uniform_frame(gs, ref, 0, 1, tiles, (14, 4), "15 tiles after the largest launch")
    shim.rt_hip_release_cache()
    _split_is_the_uniform_frame(gs, ref, 0, 1, tiles, (7, 4), "15 tiles after the release")


def test_workspace_is_handed_between_streams(gpu):
    """frame A (40 x 24, 64 spp, split 7 + 8 x 4) on one stream, frame B (37 x 21, ragged) on a second, A again on the first, nothing
    synchronised in between: every launch clears and fills the one workspace of the device, so each must wait for the event
    recorded behind the launch before it (grid_tail_ws, `t.used && t.stream != stream`).  This cannot PROVE the ordering -- a launch
    that did not wait may still happen to run after the other has resolved --, but a missing wait lets a launch clear the records
    another is summing into, and most runs would show it; the test runs once and is not looped to raise the odds"""
    import torch
    sc_a, gs_a, tiles_a, ref_a = _room(gpu, 40, 24, 64)
    sc_b, gs_b, tiles_b, ref_b = _room(gpu, 37, 21, 64)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()

    def bufs(n):
        return (torch.empty((n, 64, 3), dtype=torch.float32, device="cuda"), torch.empty((n, 64, 3), dtype=torch.uint8, device="cuda"),
                torch.zeros(4, dtype=torch.int64, device="cuda"))
    out = [bufs(tiles_a), bufs(tiles_b), bufs(tiles_a)]
    _launch(gs_a, 0, 1, tiles_a, (7, 4))   # the workspace exists and is large enough: no launch below drains the device for it
    torch.cuda.synchronize()
    before = _mixed_count()
    with _env(RT_HIP_GRID_SPLIT="7,4"):
        for (gs, n, stream), (t, t8, st) in zip(((gs_a, tiles_a, s1), (gs_b, tiles_b, s2), (gs_a, tiles_a, s1)), out):
            with torch.cuda.stream(stream):
                gs.render_tiles(SEED, 0, 1, n, tiles=t, tiles8=t8, stats=st)
    torch.cuda.synchronize()
    assert _mixed_count() - before == 3
    for (t, t8, st), ref, what in zip(out, (ref_a, ref_b, ref_a), ("A on the first stream", "B on the second", "A again")):
        _same((t.cpu().numpy().view(np.uint32), t8.cpu().numpy(), st.cpu().tolist()), ref, what)


# ---- 5. the rule, unforced, at its edges ----------------------------------------------------------------------------------------
def _takes_mixed(gs, count, bufs):
    """does an unforced launch over slots 0 .. count - 1 take the mixed form?  (no frame is read)"""
    import torch
    before = _mixed_count()
    gs.render_tiles(SEED, 0, 1, count, tiles=bufs[0], tiles8=bufs[1], stats=bufs[2])
    torch.cuda.synchronize()
    return _mixed_count() - before == 1


def _threshold(gpu):
    """T: the smallest count at which a launch of the 1,080p scene at 512 spp over tiles 0 .. count - 1 takes the mixed form,
    bisected with the counter (the rule is `tile_count >= GRID_TAIL_MIN_ROUNDS x resident`: monotonic in the count)"""
    def make():
        import torch
        sc, gs, tiles, ref = _room(gpu, *HD)
        bufs = (torch.empty((tiles, 64, 3), dtype=torch.float32, device="cuda"), torch.empty((tiles, 64, 3), dtype=torch.uint8, device="cuda"),
                torch.zeros(4, dtype=torch.int64, device="cuda"))
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        lo, hi = MIN_ROUNDS * cus - 1, tiles          # the rule cannot hold below one workgroup a CU x 8 rounds
        assert not _takes_mixed(gs, lo, bufs) and _takes_mixed(gs, hi, bufs), "the bracket [8 x CUs - 1, 32,400] does not hold the threshold"
        launches = 2
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (lo, mid) if _takes_mixed(gs, mid, bufs) else (mid, hi)
            launches += 1
        assert launches <= 18
        return hi, bufs
    return _cached("threshold", make)


def test_threshold_in_tiles_is_eight_rounds_of_resident_workgroups(gpu):
    """pt_resident_workgroups (pt_kernel.hip) states: `cus * n`, the device's CUs x hipOccupancyMaxActiveBlocksPerMultiprocessor
    of the member with the launch's LDS; grid_split_for: mixed from `tile_count >= GRID_TAIL_MIN_ROUNDS * resident` on.  So the
    threshold T is 8 R, and R a positive multiple of the CU count.  (DESIGN.md quotes R = 1,280 from a profile; R is printed here
    and not compared with a literal.)"""
    import torch
    T, _ = _threshold(gpu)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    print(f"mixed-grid threshold T = {T} tiles; R = T / {MIN_ROUNDS} = {T / MIN_ROUNDS:g} resident workgroups on {cus} CUs")
    assert T % MIN_ROUNDS == 0, T
    R = T // MIN_ROUNDS
    assert R > 0 and R % cus == 0, (R, cus)


def test_counts_around_the_threshold(gpu):
    """T - 1 stays uniform, T is mixed, both are their uniform launches; three counts above (the whole frame among them) are
    mixed, three below are not"""
    sc, gs, tiles, ref = _room(gpu, *HD)
    T, bufs = _threshold(gpu)
    import torch
    for count, mixed in ((T - 1, False), (T, True)):
        uni = _launch(gs, 0, 1, count)
        assert not uni[3] and np.array_equal(uni[0], ref[0][:count])
        before = _mixed_count()
        t, t8, st = gs.render_tiles(SEED, 0, 1, count)
        torch.cuda.synchronize()
        assert (_mixed_count() - before == 1) == mixed, f"count {count}: mixed is not {mixed}"
        _same((t.cpu().numpy().view(np.uint32), t8.cpu().numpy(), st.cpu().tolist()), uni, f"count {count}")
    for count in (T + 1, (T + tiles) // 2, tiles):
        assert _takes_mixed(gs, count, bufs), f"count {count} above T = {T} stayed uniform"
    torch.cuda.synchronize()
    assert np.array_equal(bufs[0].cpu().numpy().view(np.uint32), ref[0]) and np.array_equal(bufs[1].cpu().numpy(), ref[1]), \
        "the whole frame by the rule's own split is not the uniform frame"
    for count in (T - 2, T // 2, MIN_ROUNDS):
        assert not _takes_mixed(gs, count, bufs), f"count {count} below T = {T} took the mixed form"


def test_a_multi_device_share_by_the_rule(gpu):
    """what device 1 of 2 renders: first 1, stride 2, count 16,200.  The rule reads the slots, not the tiles: mixed if and only if
    16,200 >= T.  Its own uniform launch, and tiles 1::2 of the whole uniform frame"""
    import torch
    sc, gs, tiles, ref = _room(gpu, *HD)
    T, _ = _threshold(gpu)
    count = tiles // 2
    assert count == 16200
    uni = _launch(gs, 1, 2, count)
    assert not uni[3]
    assert np.array_equal(uni[0], ref[0][1::2]) and np.array_equal(uni[1], ref[1][1::2]), "the share's uniform launch is not the frame's tiles"
    before = _mixed_count()
    t, t8, st = gs.render_tiles(SEED, 1, 2, count)
    torch.cuda.synchronize()
    assert (_mixed_count() - before == 1) == (count >= T), f"share of {count} slots, T = {T}"
    _same((t.cpu().numpy().view(np.uint32), t8.cpu().numpy(), st.cpu().tolist()), uni, "the strided share")


def test_mixed_launch_without_bytes_and_counters(gpu):
    """rt_hip_render_tiles with d_tiles_rgb8 = NULL and d_stats = NULL under split 7 + 8 x 4: the whole slots' epilogue and
    pt_resolve_tiles both leave them alone, the floats are the uniform frame's, and 64 words of canaries on either side of the
    float buffer are untouched"""
    import torch
    sc, gs, tiles, ref = _room(gpu, 40, 24, 64)
    guard, canary = 64, 0x5CA1AB1E
    words = tiles * 64 * 3
    buf = torch.full((guard + words + guard,), canary, dtype=torch.int32, device="cuda")
    p = gs.params(SEED, 0, 1, tiles)
    torch.cuda.synchronize()
    before = _mixed_count()
    with _env(RT_HIP_GRID_SPLIT="7,4"):
        rc = gs.shim.rt_hip_render_tiles(gs.handle, C.byref(sc.camera), C.byref(p), buf.data_ptr() + 4 * guard, None, None,
                                         C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, gs.shim.rt_hip_last_error()
    torch.cuda.synchronize()
    assert _mixed_count() - before == 1
    assert gs.launch_status() == 0
    got = buf.cpu().numpy().view(np.uint32)
    assert (got[:guard] == canary).all() and (got[guard + words:] == canary).all(), "a canary beside the float buffer was written"
    assert np.array_equal(got[guard:guard + words].reshape(tiles, 64, 3), ref[0]), "floats without bytes and counters"


# ---- 6. the host form -----------------------------------------------------------------------------------------------------------
def _host_frame(gpu, sc, n_devices, uniform=False):
    """rt_hip_render_image -> (float bits, bytes, counters, mixed launches it made)"""
    before = _mixed_count()
    if uniform:
        with _env(RT_HIP_GRID_UNIFORM=1):
            img, img8, st, _ = gpu.render_image_host(sc, SEED, n_devices=n_devices)
    else:
        img, img8, st, _ = gpu.render_image_host(sc, SEED, n_devices=n_devices)
    return img.view(np.uint32), img8, st, _mixed_count() - before


def _host_same(got, ref, what):
    assert np.array_equal(got[0], ref[0]), f"{what}: floats differ"
    assert np.array_equal(got[1], ref[1]), f"{what}: bytes differ"
    assert got[2] == ref[2], f"{what}: counters {got[2]} != {ref[2]}"


def _qualifying_shares(gpu, tiles, n_devices, samples, depth):
    """how many logical devices' launches of rt_hip_render_image take the mixed form, from what the code states: device g renders
    ceil((tiles - g) / G) slots in one launch (no cancel flag: one slab); image_launch_shares asks rt_hip_suggest_chunks_depth for
    the share's chunks, and only a one-chunk launch without a workspace has the form that takes a split; the rule then asks for
    T slots"""
    T, _ = _threshold(gpu)
    gs = _room(gpu, *HD)[1]
    n = 0
    for g in range(n_devices):
        share = (tiles - g + n_devices - 1) // n_devices
        asked = int(gs.shim.rt_hip_suggest_chunks_depth(gs.handle, share, samples, depth))
        print(f"logical device {g} of {n_devices}: {share} slots, the host form asks {asked} chunk(s), T = {T}")
        n += asked == 1 and share >= T
    return n


def _host_uniform_1080p(gpu):
    return _cached("host uniform 1080p", lambda: _host_frame(gpu, _room(gpu, *HD)[0], 1, uniform=True))


@pytest.fixture
def host(gpu):
    """the cached context dropped before and after, no cancel flag (a flag would cut the frame into slabs), the identity map"""
    shim = gpu.abi.load_shim()
    shim.rt_hip_set_cancel_flag(None)
    shim.rt_hip_set_device_map(None, 0)
    shim.rt_hip_release_cache()
    yield shim
    shim.rt_hip_set_device_map(None, 0)
    shim.rt_hip_release_cache()


def test_host_form_takes_the_mixed_grid(gpu, host):
    """rt_hip_render_image on one device at 1,080p, 512 spp, no chunk workspace held: its one launch (one chunk asked, d.ws null, on
    the context's own stream) takes the mixed form, and the frame is the one the same call returns under RT_HIP_GRID_UNIFORM=1"""
    sc, gs, tiles, ref = _room(gpu, *HD)
    expected = _qualifying_shares(gpu, tiles, 1, sc.samples, sc.max_depth)
    assert expected == 1, "32,400 slots at one chunk: the premise of this test"
    uni = _host_uniform_1080p(gpu)
    assert uni[3] == 0
    host.rt_hip_release_cache()
    got = _host_frame(gpu, sc, 1)
    assert got[3] == expected
    _host_same(got, uni, "rt_hip_render_image, one device")
    assert uni[2]["samples"] == sc.width * sc.height * sc.samples


def test_host_form_two_logical_devices_on_one_gpu(gpu, host):
    """rt_hip_set_device_map((0, 0), 2): each logical device renders its strided share on a stream of its own.  The shim keeps the
    mixed grid's workspace under the scene's device, which is the PHYSICAL index (rt_hip_scene_create_opts(..., phys[g], ...)), so
    two mixed shares here are ONE workspace handed between two streams, not two workspaces.  The counter rises by the shares that
    qualify -- a share qualifies when the host form asks one chunk for it and it has T slots.
    At 1,080p each share is 16,200 slots, above T, but rt_hip_suggest_chunks_depth asks 2 chunks for a share below 100 workgroups
    a CU, so the host form renders it as its own uniform chunked launch: the count that follows from the code is 0 wherever
    16,200 < 100 x CUs.  At 2,560 x 1,440 a share is 28,800 slots, one chunk is asked, and both shares go mixed on the one
    workspace, the second waiting for the first's event.  Both frames are bit for bit the uniform ones."""
    from rt_amd import scene as S
    sc, gs, tiles, ref = _room(gpu, *HD)
    uni = _host_uniform_1080p(gpu)
    arr = (C.c_int * 2)(0, 0)
    try:
        assert host.rt_hip_set_device_map(arr, 2) == 0, host.rt_hip_last_error()
        expected = _qualifying_shares(gpu, tiles, 2, sc.samples, sc.max_depth)
        got = _host_frame(gpu, sc, 2)
        print(f"1,080p over two logical devices: {got[3]} mixed launch(es), {expected} expected")
        assert got[3] == expected
        _host_same(got, uni, "1,080p, two logical devices on one GPU")
        big = S.build_scene(4, 2560, 1440, 512)
        big_tiles = gpu.n_tiles(big.width, big.height)
        expected = _qualifying_shares(gpu, big_tiles, 2, big.samples, big.max_depth)
        assert expected == 2, "28,800 slots a share at one chunk each: the premise of the shared-workspace case"
        big_uni = _host_frame(gpu, big, 2, uniform=True)
        assert big_uni[3] == 0
        got = _host_frame(gpu, big, 2)
        assert got[3] == 2
        _host_same(got, big_uni, "2,560 x 1,440, two mixed shares on one workspace")
        big.free()
    finally:
        host.rt_hip_set_device_map(None, 0)


def test_host_form_after_a_chunked_frame(gpu, host):
    """a small frame first, for which the host form asks chunks > 1 and allocates its context's chunk workspace (d.ws); then the
    1,080p frame.  Whether the second frame still goes mixed is recorded, not asserted (the context is rebuilt when the image size
    changes, and with it d.ws; DESIGN.md, the mixed grid's open points): only the bits are"""
    from rt_amd import scene as S
    sc, gs, tiles, ref = _room(gpu, *HD)
    uni = _host_uniform_1080p(gpu)
    host.rt_hip_release_cache()
    small = S.build_scene(4, 40, 24, 256)
    sgs = gpu.GpuScene(small)
    assert sgs.suggest_chunks(15) > 1
    sgs.close()
    first = _host_frame(gpu, small, 1)
    assert first[3] == 0
    small.free()
    got = _host_frame(gpu, sc, 1)
    print(f"1,080p after a chunked 40 x 24 frame: {got[3]} mixed launch(es)")
    _host_same(got, uni, "1,080p after a chunked frame")


def test_zz_close_the_scenes(gpu):
    """the module's scenes, closed; nothing of the device is left marked failed"""
    flags = C.c_uint32(7)
    assert gpu.abi.load_shim().rt_hip_launch_status(0, C.byref(flags)) == 0 and flags.value == 0
    for name, v in list(_CACHE.items()):
        if isinstance(v, tuple) and len(v) == 4 and hasattr(v[1], "close"):
            v[1].close()
            v[0].free()
        del _CACHE[name]

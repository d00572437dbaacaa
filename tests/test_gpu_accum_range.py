"""Accumulations (rt_hip_accum_*) at the edges of the radiance range: one row per sum form an accumulation can hold -- fixed point
under a sum-bound scale, windowed words taken because of the budget alone, windowed and fp64 sums under hidden, visible and
negative emitters, the parked-walk member, and the largest budget the shim accepts (accum_range_scenes.ACCUM_ROWS;
tests/test_accum_range_cpu.py shows that each row reaches the kernel and the scale it claims).  No budget is rendered to its end:
every row is compared after 3 and 7 samples, where the plan, the sum form and the fixed-point scale are the BUDGET's and the
divisor is the COUNT's.  The floor on |got - oracle| is absolute, 1e-9, and does not follow the emitter or the budget.
"""
import numpy as np
import pytest

import accum_range_scenes as A
from conftest import SEED
from util import acc_scale_exp, assert_parity, tile_pixels, untile_numpy

pytestmark = pytest.mark.gpu

FLOOR = 1e-9   # absolute, as in tests/test_gpu_sum_range.py
ROWS = list(A.ACCUM_ROWS)


@pytest.fixture(scope="module")
def gpu():
    import torch
    from rt_amd import abi, gpu as G
    assert abi.load_shim().rt_hip_device_count() >= 1, "no HIP device: the GPU tests must run on the GPU box"
    assert torch.cuda.is_available()
    return G


def _open(gpu, row):
    """-> (scene, GpuScene, budget, the row's record)"""
    r = A.ACCUM_ROWS[row]
    sc = r["scene"]()
    return sc, gpu.GpuScene(sc), r["budget"](sc), r


def _run(gs, budget, passes, first=0, stride=1, count=None, freeze_after_first=None):
    """an accumulation of `budget` added to in `passes` -> (frames: count -> (tiles as uint32 bits, tiles8), counters after each
    pass, kernel, tile sample counts); freeze_after_first: a keep mask frozen after the first pass"""
    import torch
    acc = gs.accumulate(SEED, budget, first=first, stride=stride, count=count)
    stats = torch.zeros(4, dtype=torch.int64, device=torch.device("cuda", gs.device))
    frames, counters = {}, {}
    for i, n in enumerate(passes):
        acc.add(n, stats)
        t, t8 = acc.resolve()
        torch.cuda.synchronize()
        frames[acc.samples] = (t.cpu().numpy().view(np.uint32), t8.cpu().numpy())
        counters[acc.samples] = stats.cpu().tolist()
        if i == 0 and freeze_after_first is not None:
            assert acc.freeze(mask=freeze_after_first) == int(freeze_after_first.sum())
    kernel, counts = acc.kernel, acc.tile_samples()
    acc.close()
    return frames, counters, kernel, counts


def _image(frame, sc, total):
    t, t8 = frame
    w, h = sc.width, sc.height
    return (untile_numpy(t.view(np.float32), w, h, 0, 1, total, np.zeros((h, w, 3), np.float32)),
            untile_numpy(t8, w, h, 0, 1, total, np.zeros((h, w, 3), np.uint8)))


def _partial_frames_are_the_oracle_s(gpu, pt, sc, gs, budget, kernel, what, hdr=False):
    """(a): passes [3, 4]; resolve() after 3 and after 7 samples against the oracle's frame of that many samples"""
    total = gpu.n_tiles(sc.width, sc.height)
    frames, counters, name, _ = _run(gs, budget, [3, 4])
    assert name == kernel, f"{what}: accumulated by {name}, expected {kernel}"
    worst = 0.0
    for k in (3, 7):
        img, img8 = _image(frames[k], sc, total)
        mean, rgb8, ost = pt.render_pixels(sc, SEED, spp=k)
        st = dict(zip(("rays", "casts", "tests", "samples"), counters[k]))
        assert st["samples"] == sc.width * sc.height * k
        worst = max(worst, float(np.abs(img.astype(np.float64).reshape(-1, 3) - np.asarray(mean).reshape(-1, 3)).max()))
        assert_parity(img, img8, st, mean, rgb8, ost, what=f"{what} after {k} of {budget}", hdr=hdr, abs_floor=FLOOR)
    assert gs.launch_status() == 0
    print(f"{what}: kernel {name}, budget {budget}, scale exponents {acc_scale_exp(sc, budget)} / {acc_scale_exp(sc, 4)} (budget / pass), "
          f"worst |got - oracle| {worst:.3e} (floor {FLOOR:g}, largest value {float(np.abs(mean).max()):.3e})")
    return frames


def _schedules_agree(gs, budget, kernel, what, known=None):
    """(b): [3, 4], [7] and [1, 1, 5] at the same budget: floats and bytes at every common count, bit for bit"""
    runs = [known] if known is not None else []
    for passes in ([3, 4], [7], [1, 1, 5])[len(runs):]:
        frames, _, name, _ = _run(gs, budget, passes)
        assert name == kernel
        runs.append(frames)
    common = 0
    for i, a in enumerate(runs):
        for b in runs[i + 1:]:
            for k in set(a) & set(b):
                assert np.array_equal(a[k][0], b[k][0]) and np.array_equal(a[k][1], b[k][1]), f"{what}: schedules differ after {k} samples"
                common += 1
    assert common >= 3   # 7 three times (three pairs); 1 and 3 belong to one schedule each
    assert gs.launch_status() == 0


@pytest.mark.parametrize("row", ROWS)
def test_partial_frames_are_the_oracle_s_and_schedules_agree(gpu, pt, row):
    sc, gs, budget, r = _open(gpu, row)
    frames = _partial_frames_are_the_oracle_s(gpu, pt, sc, gs, budget, r["kernel"], row, hdr=bool(r.get("hdr")))
    _schedules_agree(gs, budget, r["kernel"], row, known=frames)
    gs.close()
    sc.free()


@pytest.mark.parametrize("row", A.SMALL_ROWS)
def test_small_budgets_end_at_the_one_shot_frame(gpu, row):
    """(c): where the budget is 16, passes [1, 2, 13] end at the chunked one-shot frame of 16 spp bit for bit, counters and member too"""
    import torch
    sc, gs, budget, r = _open(gpu, row)
    assert budget == 16
    total = gpu.n_tiles(sc.width, sc.height)
    t, t8, st = gs.render_tiles(SEED, 0, 1, total, samples=16, chunks=gs.suggest_chunks(total, 16))
    torch.cuda.synchronize()
    one_shot_kernel = gs.last_launch_kernel()
    frames, counters, name, _ = _run(gs, 16, [1, 2, 13])
    assert name == one_shot_kernel == r["kernel"], (row, name, one_shot_kernel)
    assert np.array_equal(frames[16][0], t.cpu().numpy().view(np.uint32)) and np.array_equal(frames[16][1], t8.cpu().numpy()), row
    assert counters[16] == st.cpu().tolist(), (row, counters[16], st.cpu().tolist())
    assert gs.launch_status() == 0
    gs.close()
    sc.free()


@pytest.mark.parametrize("row", ROWS)
def test_frozen_slots_hold_the_uniform_accumulation_s_bits(gpu, row):
    """(d): every third tile frozen after the first pass (rt_hip_accum_freeze_mask through Accumulation.freeze, as the imposed masks
    of tests/test_gpu_adaptive.py), then the rest of the passes: each slot's floats and bytes are the uniform accumulation's of the
    same budget after that slot's count, and rt_hip_accum_tile_samples reports those counts"""
    sc, gs, budget, r = _open(gpu, row)
    total = gpu.n_tiles(sc.width, sc.height)
    keep = np.arange(total) % 3 != 0
    uniform, _, name, ucounts = _run(gs, budget, [3, 4])
    frozen, _, fname, counts = _run(gs, budget, [3, 4], freeze_after_first=keep)
    assert name == fname == r["kernel"]
    assert (ucounts == 7).all() and np.array_equal(counts, np.where(keep, 7, 3).astype(np.uint32))
    t, t8 = frozen[7]
    for k in range(total):
        ut, ut8 = uniform[int(counts[k])]
        assert np.array_equal(t[k], ut[k]) and np.array_equal(t8[k], ut8[k]), (row, k, int(counts[k]))
    # the frozen slots differ from the live ones' count: a resolve that divided every slot by one count would not pass
    assert any(not np.array_equal(uniform[3][0][k], uniform[7][0][k]) for k in range(0, total, 3))
    assert gs.launch_status() == 0
    gs.close()
    sc.free()


@pytest.mark.parametrize("row", [k for k, r in A.ACCUM_ROWS.items() if r.get("subset")])
def test_read_image_of_a_tile_subset(gpu, row):
    """(e): rt_hip_accum_read_image of an accumulation over tiles 1, 4, 7, ...: the subset's pixels are the whole-frame
    accumulation's, bit for bit, and every other pixel is 0"""
    from rt_amd import abi
    shim = abi.load_shim()
    sc, gs, budget, r = _open(gpu, row)
    w, h = sc.width, sc.height
    total = gpu.n_tiles(w, h)
    first, stride = 1, 3
    count = (total - first + stride - 1) // stride
    whole, _, name, _ = _run(gs, budget, [3, 4])
    acc = gs.accumulate(SEED, budget, first=first, stride=stride, count=count)
    assert acc.kernel == name == r["kernel"]
    inside = np.zeros(w * h, dtype=bool)
    inside[tile_pixels(w, h, [first + k * stride for k in range(count)])] = True
    for n in (3, 4):
        acc.add(n)
        img = np.full((h, w, 3), -1.0, dtype=np.float32)
        img8 = np.full((h, w, 3), 7, dtype=np.uint8)
        assert shim.rt_hip_accum_read_image(acc.handle, img.ctypes.data, img8.ctypes.data) == 0, shim.rt_hip_last_error()
        want, want8 = _image(whole[acc.samples], sc, total)
        got, got8 = img.view(np.uint32).reshape(-1, 3), img8.reshape(-1, 3)
        assert np.array_equal(got[inside], want.view(np.uint32).reshape(-1, 3)[inside]), (row, acc.samples)
        assert np.array_equal(got8[inside], want8.reshape(-1, 3)[inside]), (row, acc.samples)
        assert not got[~inside].any() and not got8[~inside].any() and got[inside].any(), (row, acc.samples)
    acc.close()
    gs.close()
    sc.free()


def test_the_largest_budget(gpu, pt):
    """2^31 - 1 and the powers of two below it: a budget the shim refuses is a clean RT_HIP_EINVAL with no accumulation; the first it
    accepts is at least 2^24; on it the partial frames are the oracle's and the schedules agree"""
    import ctypes as C
    from rt_amd import abi
    shim = abi.load_shim()
    sc = A.LARGEST["scene"]()
    gs = gpu.GpuScene(sc)
    total = gpu.n_tiles(sc.width, sc.height)
    accepted, refused = None, []
    for budget in A.largest_candidates():
        p = gs.params(SEED, 0, 1, total, samples=budget)
        out = C.c_void_p()
        rc = shim.rt_hip_accum_create(gs.handle, C.byref(sc.camera), C.byref(p), C.byref(out))
        if rc == 0:
            assert out.value
            shim.rt_hip_accum_destroy(out)
            accepted = budget
            break
        assert rc == abi.EINVAL and not out.value, f"budget {budget}: {rc}, {shim.rt_hip_last_error()}"
        refused.append(budget)
    assert accepted is not None and accepted >= A.LARGEST["at_least"], (accepted, refused)
    with pytest.raises(gpu.ShimError, match=r"\(-2\)"):
        gs.accumulate(SEED, accepted * 2 if accepted < 2 ** 30 else 2 ** 31 - 1)
    print(f"largest accepted budget: {accepted} (refused: {refused})")
    frames = _partial_frames_are_the_oracle_s(gpu, pt, sc, gs, accepted, A.LARGEST["kernel"], "largest budget")
    _schedules_agree(gs, accepted, A.LARGEST["kernel"], "largest budget", known=frames)
    gs.close()
    sc.free()


def test_nan_stays_sticky_under_a_coarse_scale(gpu):
    """the NaN-sample scene of tests/test_gpu_edges.py with a hidden emitter of 1e9: the accumulation takes the windowed words; a
    poisoned pixel is NaN (255 in the bytes) after every later pass and in a frozen slot.  The reference stops at such a sample
    (vec3_normalize asserts), so the other pixels are compared with the same scene without the emitter, summed in fixed point:
    the same samples through the other sum form, inside the absolute floor"""
    budget, passes = 9, [1, 2, 4, 2]
    bright, dark = A.nan_scene(1e9, budget), A.nan_scene(None, budget)
    gb, gd = gpu.GpuScene(bright), gpu.GpuScene(dark)
    total = gpu.n_tiles(bright.width, bright.height)
    fb, cb, kb, _ = _run(gb, budget, passes)
    fd, cd, kd, _ = _run(gd, budget, passes)
    assert kb == "pt_render_tiles_refr_pool" and kd == "pt_render_tiles"
    before = None
    for k in (1, 3, 7, 9):
        f, f8 = fb[k][0].view(np.float32), fb[k][1]
        d = fd[k][0].view(np.float32)
        nan = np.isnan(f)
        assert np.array_equal(nan, np.isnan(d)), f"the sum forms disagree on the NaN pixels after {k} samples"
        assert (f8[nan] == 255).all()
        assert before is None or (nan | ~before).all(), f"a NaN pixel turned finite after {k} samples"
        err = np.abs(f[~nan].astype(np.float64) - d[~nan].astype(np.float64))
        assert (err <= 1e-6 * np.abs(d[~nan]) + FLOOR).all(), (k, float(err.max()))
        assert cb[k][:2] == cd[k][:2] and cb[k][3] == cd[k][3]     # rays, casts, samples (tests: the bright scene has two more spheres)
        before = nan
    assert before.any() and not before.all() and np.isnan(fb[3][0].view(np.float32)).any()
    # frozen after the first pass: a poisoned pixel of a frozen slot stays NaN, and the slot is the uniform one's at its count
    keep = np.arange(total) % 3 != 0
    ff, _, _, counts = _run(gb, budget, passes, freeze_after_first=keep)
    assert np.array_equal(counts, np.where(keep, 9, 1).astype(np.uint32))
    nan1 = np.isnan(fb[1][0].view(np.float32))
    assert nan1[~keep].any(), "a frozen slot should hold a poisoned pixel"
    for k in range(total):
        assert np.array_equal(ff[9][0][k], fb[int(counts[k])][0][k]) and np.array_equal(ff[9][1][k], fb[int(counts[k])][1][k]), k
    assert np.isnan(ff[9][0].view(np.float32))[~keep][nan1[~keep]].all()
    assert gb.launch_status() == 0
    for g in (gb, gd):
        g.close()
    bright.free()
    dark.free()

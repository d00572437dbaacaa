"""Adaptive sampling without a GPU: the numpy restatement of the contract (tests/adaptive_expected.py) against the scalar one
on hostile buffers, the pass schedule (also the shim's own rt_hip_adapt_schedule, which needs no device), and the ABI."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import adaptive_expected as ae

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLT_MAX = np.finfo(np.float32).max
DENORM = np.float32(1e-45)


def hostile_buffers(rng, count):
    """cur, prev [count, 64, 3] float32 with NaN / inf pixels, negative channels, -0.0, denormals and FLT_MAX sprinkled in"""
    cur = rng.random((count, 64, 3), dtype=np.float32) * np.float32(2.0)
    prev = cur + (rng.random((count, 64, 3), dtype=np.float32) - np.float32(0.5)) * np.float32(0.2)
    special = np.array([np.nan, np.inf, -np.inf, -1.5, -0.0, 0.0, DENORM, -DENORM, FLT_MAX, -FLT_MAX], dtype=np.float32)
    for buf in (cur, prev):
        hit = rng.random(buf.shape) < 0.03
        buf[hit] = special[rng.integers(0, len(special), size=int(hit.sum()))]
    if count > 2:
        cur[1], prev[1] = np.float32(-0.25), np.float32(-0.5)      # a tile of negative channels: l clamps to 0
        # cur = -FLT_MAX against prev = +FLT_MAX: l clamps to 0 and E = 192 FLT_MAX overflows float32 to +inf (the other way
        # round l = 3 FLT_MAX and E stays finite, about 6.4e19): either way the tile is kept
        cur[2, :, :], prev[2, :, :] = -FLT_MAX, FLT_MAX
    return cur, prev


CASES = [(1, 1, 0, 1, None), (9, 9, 0, 1, None), (37, 21, 0, 1, None), (160, 96, 0, 1, None), (37, 21, 1, 3, None),
         (64, 57, 2, 3, None), (15, 63, 0, 1, None), (8, 8, 0, 1, None)]


def case_count(w, h, first, stride):
    tx, ty = ae.tile_grid(w, h)
    return (tx * ty - first + stride - 1) // stride


@pytest.mark.parametrize("w,h,first,stride,_", CASES)
def test_tile_error_numpy_equals_scalar(w, h, first, stride, _):
    count = case_count(w, h, first, stride)
    rng = np.random.default_rng(w * 1000 + h + first)
    cur, prev = hostile_buffers(rng, count)
    a = ae.tile_error(cur, prev, w, h, first, stride, count)
    b = ae.tile_error_scalar(cur, prev, w, h, first, stride, count)
    assert a.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_tile_error_known_answers():
    # one valid pixel (1x1 image): E = d / sqrt(l + eps), nothing to sum
    cur, prev = np.zeros((1, 64, 3), np.float32), np.zeros((1, 64, 3), np.float32)
    cur[0, 0], prev[0, 0] = (0.5, 0.25, 0.25), (0.25, 0.25, 0.5)
    want = np.float32(0.5 / np.sqrt(1.0 + ae.EPS))
    assert ae.tile_error(cur, prev, 1, 1, 0, 1, 1)[0] == want
    # pixels outside the image do not count, whatever they hold
    cur[0, 1:], prev[0, 1:] = np.nan, 7.0
    assert ae.tile_error(cur, prev, 1, 1, 0, 1, 1)[0] == want
    # a NaN or inf pixel inside contributes +0.0 but stays in `valid`
    cur2, prev2 = np.full((1, 64, 3), 0.5, np.float32), np.full((1, 64, 3), 0.25, np.float32)
    base = ae.tile_error(cur2, prev2, 8, 8, 0, 1, 1)[0]
    cur2[0, 5, 1] = np.inf
    assert ae.tile_error(cur2, prev2, 8, 8, 0, 1, 1)[0] == np.float32(np.float64(base) * 63 / 64)
    # negative channels: l clamps to 0, e = d / sqrt(eps) = 32 d
    c3, p3 = np.full((1, 64, 3), -0.25, np.float32), np.full((1, 64, 3), -0.5, np.float32)
    assert ae.tile_error(c3, p3, 8, 8, 0, 1, 1)[0] == np.float32(0.75 * 32)
    # FLT_MAX against -FLT_MAX: d = 6 FLT_MAX is finite in fp64 (the contract widens first), E = 2 sqrt(3 FLT_MAX): huge, kept
    c4, p4 = np.full((1, 64, 3), FLT_MAX, np.float32), np.full((1, 64, 3), -FLT_MAX, np.float32)
    e4 = ae.tile_error(c4, p4, 8, 8, 0, 1, 1)
    assert e4[0] == np.float32(6 * float(FLT_MAX) / np.sqrt(3 * float(FLT_MAX) + ae.EPS)) and e4[0] > 1e19
    assert ae.keep_mask(e4, [True], 8, 8, 0, 1, 1, 1e6, 0)[0]
    # ... the other way round l clamps to 0 and E = 192 FLT_MAX overflows float32: +inf, and !(inf <= t) keeps the tile
    e4 = ae.tile_error(p4, c4, 8, 8, 0, 1, 1)
    assert np.isposinf(e4[0]) and ae.keep_mask(e4, [True], 8, 8, 0, 1, 1, 1e30, 0)[0]
    # -0.0 and denormals are ordinary values
    c5, p5 = np.full((1, 64, 3), -0.0, np.float32), np.full((1, 64, 3), DENORM, np.float32)
    assert ae.tile_error(c5, p5, 8, 8, 0, 1, 1)[0] == np.float32(3 * float(DENORM) * 32)


@pytest.mark.parametrize("valid_w,valid_h", [(1, 1), (7, 1), (1, 7), (3, 5), (7, 7), (7, 8), (8, 7), (7, 9)])
def test_ragged_edge_tiles_divide_by_their_valid_pixels(valid_w, valid_h):
    w, h = 8 + valid_w, 8 + valid_h
    count = case_count(w, h, 0, 1)
    cur, prev = np.full((count, 64, 3), 1.0, np.float32), np.full((count, 64, 3), 0.5, np.float32)
    e = ae.tile_error(cur, prev, w, h, 0, 1, count)
    assert np.array_equal(e, ae.tile_error_scalar(cur, prev, w, h, 0, 1, count))
    assert len(set(e.tolist())) <= 2 and abs(float(e[-1]) - 1.5 / np.sqrt(3 + ae.EPS)) < 1e-6   # a mean: the same everywhere


@pytest.mark.parametrize("w,h,first,stride,_", CASES)
@pytest.mark.parametrize("dilate", [0, 1, 2])
def test_keep_mask_numpy_equals_scalar(w, h, first, stride, _, dilate):
    count = case_count(w, h, first, stride)
    rng = np.random.default_rng(dilate * 77 + w + h)
    err = rng.random(count, dtype=np.float32)
    err[rng.random(count) < 0.1] = np.nan
    err[rng.random(count) < 0.05] = np.inf
    live = rng.random(count) < 0.8
    for thr in (0.5, 0.05, 2.0, np.inf, 0.0, -1.0):
        a = ae.keep_mask(err, live, w, h, first, stride, count, thr, dilate)
        b = ae.keep_mask_scalar(err, live, w, h, first, stride, count, thr, dilate)
        assert np.array_equal(a, b)
        assert not (a & ~live).any(), "a frozen slot never comes back"
    assert np.array_equal(ae.keep_mask(err, live, w, h, first, stride, count, 0.0, dilate), live)
    finite = ae.keep_mask(np.nan_to_num(err, nan=0.0, posinf=0.0), live, w, h, first, stride, count, np.inf, dilate)
    assert not finite.any(), "threshold = +inf freezes every slot with a finite error"


def test_dilation_and_stride_neighbours():
    # 5 x 5 tiles, only the centre noisy
    err = np.zeros(25, np.float32)
    err[12] = 1.0
    live = np.ones(25, bool)
    for dilate, n in ((0, 1), (1, 9), (2, 25)):
        assert ae.keep_mask(err, live, 40, 40, 0, 1, 25, 0.5, dilate).sum() == n
    # stride 2 from tile 0: slots are tiles 0, 2, ..., 24; tile 12 = slot 6; its launched neighbours within 1 are 6, 8, 16, 18
    k = ae.keep_mask(err[::2], np.ones(13, bool), 40, 40, 0, 2, 13, 0.5, 1)
    assert sorted((np.flatnonzero(k) * 2).tolist()) == [6, 8, 12, 16, 18]


def test_freeze_is_monotone_and_the_list_ascends():
    counts = np.zeros(10, np.uint32)
    counts, lst = ae.freeze(counts, [1, 0, 1, 1, 0, 1, 1, 1, 0, 1], 16)
    assert counts.tolist() == [0, 16, 0, 0, 16, 0, 0, 0, 16, 0] and lst.tolist() == [0, 2, 3, 5, 6, 7, 9]
    counts, lst = ae.freeze(counts, [0, 1, 1, 0, 1, 1, 0, 1, 1, 1], 32)   # keeping a frozen slot does not revive it
    assert counts.tolist() == [32, 16, 0, 32, 16, 0, 32, 0, 16, 0] and lst.tolist() == [2, 5, 7, 9]


SCHEDULES = {
    (1, 1): [1], (1, 2): [1], (1, 16): [1], (1, 40): [1],
    (2, 1): [1, 2], (2, 2): [1, 2], (2, 16): [2], (2, 40): [2],
    (3, 1): [1, 2, 3], (3, 2): [1, 2, 3], (3, 16): [3], (3, 40): [3],
    (16, 1): [1, 2, 4, 8, 16], (16, 2): [1, 2, 4, 8, 16], (16, 16): [8, 16], (16, 40): [16],
    (17, 1): [1, 2, 4, 8, 16, 17], (17, 2): [1, 2, 4, 8, 16, 17], (17, 16): [8, 16, 17], (17, 40): [17],
    (1000, 1): [1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1000], (1000, 2): [1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1000],
    (1000, 16): [8, 16, 32, 64, 128, 256, 512, 1000], (1000, 2000): [1000],
}


@pytest.mark.parametrize("budget,min_samples", sorted(SCHEDULES))
def test_schedule(budget, min_samples):
    want = SCHEDULES[(budget, min_samples)]
    assert ae.schedule(budget, min_samples) == want
    assert ae.checkpoints(budget, min_samples) == want[1:-1]
    if min_samples % 2 == 0 and min_samples <= budget:   # checkpoints at min_samples * 2^j below the budget
        assert all(c == min_samples << j for j, c in enumerate(ae.checkpoints(budget, min_samples)))
    from rt_amd import abi
    assert abi.adapt_schedule(budget, min_samples) == want, "the shim's own schedule"


def test_schedule_of_nothing():
    from rt_amd import abi
    assert ae.schedule(0, 16) == [] and ae.schedule(16, 0) == []
    assert abi.adapt_schedule(0, 16) == [] and abi.adapt_schedule(16, 0) == []
    assert len(abi.adapt_schedule(2 ** 31 - 1, 1)) == 32


def test_abi_struct_and_defaults():
    from rt_amd import abi
    assert C.sizeof(abi.RtHipAdaptParams) == 16
    assert (abi.RtHipAdaptParams.min_samples.offset, abi.RtHipAdaptParams.dilate.offset, abi.RtHipAdaptParams.threshold.offset) == (0, 4, 8)
    p = abi.adapt_params()
    assert (p.min_samples, p.dilate, p.threshold) == (16, 1, 0.02)
    assert abi.adapt_params(min_samples=4, threshold=0.5, dilate=0).min_samples == 4
    header = open(os.path.join(ROOT, "include", "rt_hip.h")).read()
    body = re.search(r"typedef struct\s*\{([^}]*)\}\s*RtHipAdaptParams;", header).group(1)
    fields = re.findall(r"\b(?:int32_t|uint32_t|double)\s+(\w+)\s*;", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == [f for f, _ in abi.RtHipAdaptParams._fields_]
    for name in ("rt_hip_tile_error", "rt_hip_accum_freeze", "rt_hip_accum_freeze_mask", "rt_hip_accum_tile_samples",
                 "rt_hip_accum_live_tiles", "rt_hip_accum_run_adaptive", "rt_hip_adapt_defaults", "rt_hip_adapt_schedule",
                 "rt_hip_render_adaptive_image"):
        assert name in abi.SHIM_SYMBOLS and re.search(r"\b%s\s*\(" % name, header)


def test_argument_checks_come_before_the_device():
    """RT_HIP_EINVAL for bad arguments with or without a GPU (then RT_HIP_ENODEV), as rt_hip_denoise does"""
    from rt_amd import abi
    shim = abi.load_shim()
    buf = (C.c_float * 192)()
    assert shim.rt_hip_tile_error(None, buf, 8, 8, 0, 1, 1, buf, None) == -2
    assert shim.rt_hip_tile_error(buf, buf, 0, 8, 0, 1, 1, buf, None) == -2
    assert shim.rt_hip_tile_error(buf, buf, 8, 8, 1, 1, 1, buf, None) == -2       # tile outside the image
    assert shim.rt_hip_tile_error(buf, buf, 16, 8, 0, 0, 2, buf, None) == -2      # stride 0 with two tiles
    assert shim.rt_hip_accum_freeze(None, buf, 0.5, 1, None, None) == -2
    assert shim.rt_hip_accum_freeze_mask(None, buf, None, None) == -2
    assert shim.rt_hip_accum_tile_samples(None, buf) == -2
    assert shim.rt_hip_accum_run_adaptive(None, None, None, None, None, None) == -2
    assert shim.rt_hip_accum_live_tiles(None) == 0
    assert shim.rt_hip_render_adaptive_image(None, 0, None, 0, None, None, None, 0, None, None, None, None, None, None, None) == -2
    if shim.rt_hip_device_count() == 0:
        assert shim.rt_hip_tile_error(buf, buf, 8, 8, 0, 1, 1, buf, None) == abi.ENODEV
        assert shim.rt_hip_tile_error(buf, buf, 8, 8, 0, 0, 1, buf, None) == abi.ENODEV   # stride 0 with ONE tile is a valid launch
    else:
        assert shim.rt_hip_tile_error(buf, buf, 8, 8, 0, 1, 1, buf, None) == -2           # host pointers are refused, not launched

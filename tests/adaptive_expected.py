"""The adaptive-sampling contract of include/rt_hip.h (rt_hip_tile_error, rt_hip_accum_freeze, rt_hip_adapt_schedule) restated
in numpy, and once more as scalar Python written line by line from the header: tests/test_adaptive_cpu.py pins the two against
each other, tests/test_gpu_adaptive.py compares the device with the numpy form bit for bit.

Buffers are compact tile-major as rt_hip_accum_resolve writes them: slot k of the launch (tile first + k * stride of the
image's row-major 8x8 tile grid) owns floats [k * 192, (k + 1) * 192) = 64 pixels (row-major in the tile) x RGB."""
import math

import numpy as np

EPS = 2.0 ** -10
TILE = 8


def tile_grid(width, height):
    return (width + TILE - 1) // TILE, (height + TILE - 1) // TILE


def inside_mask(width, height, first, stride, count):
    """bool [count, 64]: which pixels of every slot's tile lie inside the image"""
    tx, _ = tile_grid(width, height)
    tiles = first + np.arange(count, dtype=np.int64) * stride
    px = (tiles % tx)[:, None] * TILE + (np.arange(64) & 7)[None, :]
    py = (tiles // tx)[:, None] * TILE + (np.arange(64) >> 3)[None, :]
    return (px < width) & (py < height)


def tile_error(cur, prev, width, height, first, stride, count):
    """-> float32 [count], the contract's E per slot"""
    c = np.asarray(cur, dtype=np.float32).reshape(count, 64, 3).astype(np.float64)
    p = np.asarray(prev, dtype=np.float32).reshape(count, 64, 3).astype(np.float64)
    inside = inside_mask(width, height, first, stride, count)
    ok = inside & np.isfinite(c).all(axis=2) & np.isfinite(p).all(axis=2)
    with np.errstate(all="ignore"):
        d = (np.abs(c[..., 0] - p[..., 0]) + np.abs(c[..., 1] - p[..., 1])) + np.abs(c[..., 2] - p[..., 2])
        lum = (c[..., 0] + c[..., 1]) + c[..., 2]
        lum = np.where(lum > 0, lum, 0.0)
        e = np.where(ok, d / np.sqrt(lum + EPS), 0.0)
        v = e.copy()
        m = 32
        while m >= 1:
            v[:, :m] = v[:, :m] + v[:, m:2 * m]
            m //= 2
        return (v[:, 0] / inside.sum(axis=1).astype(np.float64)).astype(np.float32)


def tile_error_scalar(cur, prev, width, height, first, stride, count):
    """the same, a pixel at a time with Python floats (IEEE doubles)"""
    cur = np.asarray(cur, dtype=np.float32).reshape(-1)
    prev = np.asarray(prev, dtype=np.float32).reshape(-1)
    tx, _ = tile_grid(width, height)
    out = np.zeros(count, dtype=np.float32)
    for k in range(count):
        tile = first + k * stride
        x0, y0 = (tile % tx) * TILE, (tile // tx) * TILE
        v, valid = [0.0] * 64, 0
        for i in range(64):
            if not (x0 + (i & 7) < width and y0 + (i >> 3) < height):
                continue
            valid += 1
            c = [float(cur[k * 192 + 3 * i + ch]) for ch in range(3)]
            p = [float(prev[k * 192 + 3 * i + ch]) for ch in range(3)]
            if not all(math.isfinite(x) for x in c + p):
                continue
            d = (abs(c[0] - p[0]) + abs(c[1] - p[1])) + abs(c[2] - p[2])
            lum = (c[0] + c[1]) + c[2]
            lum = lum if lum > 0 else 0.0
            v[i] = d / math.sqrt(lum + EPS)
        m = 32
        while m >= 1:
            for i in range(m):
                v[i] = v[i] + v[i + m]
            m //= 2
        with np.errstate(over="ignore"):
            out[k] = np.float32(v[0] / valid)
    return out


def keep_mask(error, live, width, height, first, stride, count, threshold, dilate):
    """-> bool [count]: slot k stays live iff it is live and some slot of the launch within Chebyshev distance `dilate` of its
    tile has !(E <= threshold); threshold <= 0 (or NaN) freezes nothing (rt_hip_accum_freeze)"""
    live = np.asarray(live, dtype=bool)
    if not threshold > 0:
        return live.copy()
    tx, ty = tile_grid(width, height)
    with np.errstate(invalid="ignore"):
        noisy = ~(np.asarray(error, dtype=np.float32).astype(np.float64) <= threshold)
    grid = np.zeros((ty + 2 * dilate, tx + 2 * dilate), dtype=bool)   # votes by tile, padded
    tiles = first + np.arange(count, dtype=np.int64) * stride
    gx, gy = tiles % tx + dilate, tiles // tx + dilate
    grid[gy, gx] = noisy
    vote = np.zeros(count, dtype=bool)
    for dy in range(-dilate, dilate + 1):
        for dx in range(-dilate, dilate + 1):
            vote |= grid[gy + dy, gx + dx]
    return vote & live


def keep_mask_scalar(error, live, width, height, first, stride, count, threshold, dilate):
    if not threshold > 0:
        return np.asarray(live, dtype=bool).copy()
    tx, ty = tile_grid(width, height)
    slot_of = {first + k * stride: k for k in range(count)}
    out = np.zeros(count, dtype=bool)
    for k in range(count):
        tile = first + k * stride
        x, y = tile % tx, tile // tx
        vote = False
        for dy in range(-dilate, dilate + 1):
            for dx in range(-dilate, dilate + 1):
                if not (0 <= x + dx < tx and 0 <= y + dy < ty):
                    continue
                u = slot_of.get((y + dy) * tx + x + dx)
                if u is not None and not (float(error[u]) <= threshold):
                    vote = True
        out[k] = vote and bool(live[k])
    return out


def freeze(counts, keep, done):
    """the freeze on the count map (0 = live): live slots that `keep` drops take `done` -> (counts, ascending list of live slots)"""
    counts = np.asarray(counts, dtype=np.uint32).copy()
    counts[(counts == 0) & ~np.asarray(keep, dtype=bool)] = done
    return counts, np.flatnonzero(counts == 0).astype(np.uint32)


def schedule(budget, min_samples):
    """the sample counts the passes end at (rt_hip_adapt_schedule): h = max(1, min_samples // 2), 2h, 4h, ... cut at the budget"""
    if budget < 1 or min_samples < 1:
        return []
    out, t = [], max(1, min_samples // 2)
    while True:
        out.append(min(t, budget))
        if out[-1] == budget:
            return out
        t *= 2


def checkpoints(budget, min_samples):
    """the sample counts an estimate and a freeze follow: every target but the first and the last"""
    return schedule(budget, min_samples)[1:-1]

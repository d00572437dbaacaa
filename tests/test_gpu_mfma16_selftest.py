"""Keep words of phase 1 on the fp16 matrix pipe against known answers (rt_hip_selftest_intersect kind 2: pt_selftest_mfma16 runs
filter_mfma16 and filter_chunk's merge on caller data, beside the packed sign-test form and the device's exact test).

Two blocks of 64 rays against the same 64 spheres; spheres 0..31 of a block are the matrix rows, 32..63 follow in the packed loop.
  block 0, the layout sweep: ray k hits sphere k through half its radius, ray 32 + k misses sphere k by d2 = r^2 + 2.5 W16;
  block 1, the margins (k = i % 32): 16 rays graze sphere k inside it (d2 = r^2 (1 - 1e-6)), 16 miss it inside the bound
  (d2 = r^2 + W16 / 2: either answer is right), 16 start inside sphere k, 8 have a NaN direction, 8 start beyond near_R.
What is asserted, and where the figures come from (the derivation above pt_mfma16_row, pt_device.h):
  - all rows fit, so the matrix pipe and not the packed loop gave the words (h_hit);
  - every pair the fp64 exact test accepts -- the device's exact_sphere and the oracle's intersect_sphere agree on it -- is
    kept, by the matrix form and by the packed form, for all 128 x 64 pairs;
  - the hits and grazes are exact hits and are kept, the rays inside a sphere keep it, the rays beyond near_R keep everything;
  - a miss by more than W16 + E16 (+ the split's residual) must be DROPPED: q''16 <= r^2 + W16 - d2 + E16 < 0, and E16 <= W16,
    so d2 = r^2 + 2.5 W16 is outside.  With the hits of the sweep this places every row of the A operand: a sphere in the wrong
    row would lose its hit or keep its miss;
  - the words of spheres 32..63 are the packed loop's own, bit for bit;
  - the pipe's raw tca16 and ll16 (spheres 0 and 16 against 32 rays of each block) are within ET and EL of fp64: the sum of
    sixteen exact products on the matrix pipe loses what the bound allows for and no more;
  - NaN directions hit nothing in the exact test; which bits such a ray keeps is not specified (a NaN's sign is arbitrary).
The share of exact misses that the matrix form keeps and the packed form drops is printed."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "raytracer.c_amd"))

NEAR_R = 160.0
E = 2.0 ** -24


def _spheres():
    cen, rad = [], []
    for k in range(32):      # the matrix rows: a 4 x 4 x 2 grid in the room, radii 0.5 .. 2.05
        cen.append((-27.0 + 18.0 * (k % 4), -15.0 + 10.0 * ((k // 4) % 4), -20.0 + 50.0 * (k // 16)))
        rad.append(0.5 + 0.05 * k)
    for k in range(32):      # behind them, in the packed loop
        cen.append((-30.0 + 2.0 * k, 17.0 - 0.5 * k, 5.0 + 0.25 * k))
        rad.append(0.75)
    return np.array(cen), np.array(rad)


def _bounds(cen, rad):
    """A, W16, ET, EL per sphere, as pt_mfma16_row computes them (filt_shift as the self-test's launch sets it)"""
    cn = np.linalg.norm(cen, axis=1) * (1.0 + 1e-12)
    tol = 12.0 * E * (cn.max() + NEAR_R) * (1.0 + 1e-9)
    A = (cn + NEAR_R + tol) * (1.0 + 1e-6)
    g = np.abs(cn * cn - rad * rad)
    W16 = (A * A / 65536.0 + g / 262144.0 + A / 131072.0) * (1.0 + 1e-6)
    kq = np.abs(cn * cn - rad * rad - W16)
    ET = 3 * 2.0 ** -19 * A + 2.0 ** -20
    EL = 1.82 * 2.0 ** -19 * A * A + 1.16 * 2.0 ** -19 * kq + 6 * E * A
    return tol, A, W16, ET, EL


def _frame(k):
    """a unit direction and a unit normal to it, fixed per k"""
    rng = np.random.default_rng(1000 + k)
    d = rng.normal(size=3)
    d /= np.linalg.norm(d)
    p = np.cross(d, rng.normal(size=3))
    p /= np.linalg.norm(p)
    return d, p


def _rays(cen, rad, W16):
    rays, kind = np.zeros((128, 6)), []
    for i in range(128):
        k = i % 32
        d, p = _frame(i)
        c, r = cen[k], rad[k]
        if i < 32:
            b, what = 0.5 * r, "hit"
        elif i < 64:
            b, what = np.sqrt(r * r + 2.5 * W16[k]), "miss"
        elif i < 80:
            b, what = r * np.sqrt(1.0 - 1e-6), "graze"
        elif i < 96:
            b, what = np.sqrt(r * r + 0.5 * W16[k]), "margin"
        elif i < 112:
            b, what = None, "inside"
        elif i < 120:
            b, what = 0.5 * r, "nan"
        else:
            b, what = None, "far"
        if what == "inside":
            o = c + 0.3 * r * p
        elif what == "far":
            o = c - (NEAR_R + 80.0) * d
        else:
            o = c - 10.0 * d + b * p
        if what == "nan":
            d = np.array([np.nan, d[1], d[2]]) * (-1.0 if i % 2 else 1.0)
        rays[i, :3], rays[i, 3:] = o, d
        kind.append(what)
    return rays, np.array(kind)


@pytest.fixture(scope="module")
def run():
    from rt_amd import abi
    shim = abi.load_shim()
    cen, rad = _spheres()
    tol, A, W16, ET, EL = _bounds(cen, rad)
    rays, kind = _rays(cen, rad, W16)
    prims = np.ascontiguousarray(np.tile(np.concatenate([cen, rad[:, None]], axis=1), (2, 1)))
    hit = np.zeros(128, dtype=np.uint8)
    tuv = np.zeros((128, 3))
    keep = np.zeros((128, 3), dtype=np.uint64)
    rc = shim.rt_hip_selftest_intersect(2, rays.ctypes.data, prims.ctypes.data, 128, C.c_double(NEAR_R), hit.ctypes.data, tuv.ctypes.data,
                                        keep.ctypes.data, 0)
    assert rc == 0, shim.rt_hip_last_error()
    bits = lambda col: ((keep[:, col][:, None] >> np.arange(64, dtype=np.uint64)[None]) & np.uint64(1)).astype(bool)   # noqa: E731
    return dict(cen=cen, rad=rad, tol=tol, A=A, W16=W16, ET=ET, EL=EL, rays=rays, kind=kind, hit=hit, tuv=tuv, packed=bits(0), matrix=bits(1),
                exact=bits(2))


@pytest.mark.gpu
def test_keep_words_of_the_matrix_pipe(run, pt):
    R = run
    cen, rad, rays, kind = R["cen"], R["rad"], R["rays"], R["kind"]
    assert (R["hit"] == 1).all(), "a row did not fit: the block ran the packed loop, not the matrix pipe"
    # the fp64 exact test: the oracle's intersect_sphere, and the device's exact_sphere says the same
    exact = np.array([[bool(pt.intersect_sphere(rays[i], cen[j], rad[j])[0]) for j in range(64)] for i in range(128)])
    assert np.array_equal(exact, R["exact"])
    assert not (exact & ~R["matrix"]).any(), "the matrix form drops a pair the exact test accepts"
    assert not (exact & ~R["packed"]).any()
    k = np.arange(128) % 32
    own = lambda m: m[np.arange(128), k]   # noqa: E731  (ray i, its target sphere)
    for what in ("hit", "graze"):
        assert own(exact)[kind == what].all() and own(R["matrix"])[kind == what].all(), what
    for what in ("miss", "margin", "nan"):
        assert not own(exact)[kind == what].any(), what
    assert not exact[kind == "nan"].any()
    assert own(R["matrix"])[kind == "inside"].all()
    assert R["matrix"][kind == "far"].all() and R["packed"][kind == "far"].all()
    assert not own(R["matrix"])[kind == "miss"].any(), "a miss beyond W16 + E16 is kept: a row of the A operand is misplaced, or the bound does not hold"
    assert np.array_equal(R["matrix"][:, 32:], R["packed"][:, 32:]), "the packed loop behind the matrix rows changed its words"
    near = kind != "far"
    extra = R["matrix"][near, :32] & ~R["packed"][near, :32] & ~exact[near, :32]
    print("exact misses the matrix form keeps and the packed form drops: %d of %d evaluations (%.3f %%); margin rays kept: %d of 16"
          % (extra.sum(), extra.size, 100.0 * extra.mean(), own(R["matrix"])[kind == "margin"].sum()))


@pytest.mark.gpu
def test_accumulators_of_the_matrix_pipe_are_within_the_bound(run):
    R = run
    cen, rad, rays, kind = R["cen"], R["rad"], R["rays"], R["kind"]
    worst_t = worst_l = 0.0
    for i in range(128):
        ray, s = 64 * (i // 64) + i % 32, 16 * ((i % 64) // 32)
        if kind[ray] in ("nan", "far"):
            continue
        o, d = rays[ray, :3] - R["tol"] * rays[ray, 3:], rays[ray, 3:]
        L = cen[s] - o
        tca = float(L @ d)
        assert abs(R["tuv"][i, 0] - tca) <= R["ET"][s], (i, R["tuv"][i, 0], tca)
        # ll16 stands for |c - o'|^2 - (|c|^2 - kq16), kq16 at most |c|^2 - r^2 - W16 and within 2^-20 |.| + 2^-22 of it (the row's split)
        target = float(L @ L) - rad[s] ** 2 - R["W16"][s]
        kq = abs(float(cen[s] @ cen[s]) - rad[s] ** 2 - R["W16"][s])
        err = R["tuv"][i, 1] - target
        assert -R["EL"][s] - (kq * 2.0 ** -20 + 2.0 ** -22) - 1e-9 * (1 + kq) <= err <= R["EL"][s] + 1e-9 * (1 + kq), (i, R["tuv"][i, 1], target)
        worst_t, worst_l = max(worst_t, abs(R["tuv"][i, 0] - tca) / R["ET"][s]), max(worst_l, abs(err) / R["EL"][s])
    print("largest |tca16 - tca'| / ET = %.3f, |ll16 - ll| / EL = %.3f" % (worst_t, worst_l))

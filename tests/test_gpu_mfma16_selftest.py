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
The share of exact misses that the matrix form keeps and the packed form drops is printed.

That layout sits at one operating point (near_R = 160, radii of order 1, centres 20 to 60 out).  The SHARED SETS of
tests/mfma16_vectors.py take the same statements to the edges of the fit rule and of the bound, one self-test call per set:
near_R = 250 and the next double after it (no row may fit), the layout scaled down to near_R = 2^-6 (centre halves below 2^-14: fp16
subnormals, where the phi floors of the derivation carry the bound), signed zeros and components of 2^-15 and 2^-20, concentric and
identical spheres, a radius of 1e-100, |kq| near 60000 beside the twins that just do not fit, and a call whose middle block alone
has an unfitting row.  Per set:
  - h_hit per block as the set states; where it is 0 the matrix words ARE the packed words;
  - no pair the device's exact test accepts is dropped by either form (no tolerance), and that test equals the oracle's;
  - hits, grazes and axis rays keep their sphere, rays inside one keep it, rays beyond near_R and in the far-origin shell
    (|o| = near_R (1 - 2^-20): filter_ray turns away |o'|^2 > 0.9999 near_R^2) keep everything, surface origins lose nothing exact;
  - the aimed misses are dropped.  They stand at r^2 + 2.5 W16 where E16 < 1.5 W16 - (the split's residual) holds for every row of
    the set -- asserted from the formulas first -- and else (near_R = 2^-6: the constant 2^-22 of the residual outweighs W16 / 2
    there) at r^2 + W16 + residual + 1.25 E16, from E16's formula; never from what the device returns;
  - raw tca16 and ll16 within ET and EL on every fitting block (spheres 0 and 16 of the block against its lanes 0..31)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "raytracer.c_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mfma16_vectors as V   # noqa: E402

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
    """A, W16, ET, EL per sphere (tests/mfma16_vectors.py restates pt_mfma16_row's figures; filt_shift as the self-test's launch sets it)"""
    tol = V.filt_shift(float(V.center_norm(cen).max()), NEAR_R)
    B = V.bounds(cen, rad, NEAR_R, tol)
    return tol, B["A"], B["W16"], B["ET"], B["EL"]


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


# ---- the shared sets ------------------------------------------------------------------------------------------------------------
_CALLS = {}


def _call(name):
    """one rt_hip_selftest_intersect call per set, shared by the tests of that set"""
    if name not in _CALLS:
        from rt_amd import abi
        shim = abi.load_shim()
        S = V.SETS[name]
        rays, prims = V.arrays(S)
        n = len(rays)
        hit, tuv, keep = np.zeros(n, dtype=np.uint8), np.zeros((n, 3)), np.zeros((n, 3), dtype=np.uint64)
        rc = shim.rt_hip_selftest_intersect(2, rays.ctypes.data, prims.ctypes.data, n, C.c_double(S["near_R"]), hit.ctypes.data, tuv.ctypes.data,
                                            keep.ctypes.data, 0)
        assert rc == 0, shim.rt_hip_last_error()
        bits = lambda col: ((keep[:, col][:, None] >> np.arange(64, dtype=np.uint64)[None]) & np.uint64(1)).astype(bool)   # noqa: E731
        _CALLS[name] = dict(hit=hit, tuv=tuv, packed=bits(0), matrix=bits(1), exact=bits(2))
    return _CALLS[name]


def test_must_drop_inequality_of_every_set():
    """E16 < 1.5 W16 - residual, row by row, from the formulas: it holds everywhere but at near_R = 2^-6, whose misses stand at
    r^2 + W16 + residual + 1.25 E16 instead (docs/HISTORY.md: the comment's "E16 <= W16" is not general)"""
    for name, S in V.SETS.items():
        for b in S["blocks"]:
            B = {k: v[:32] for k, v in b["bounds"].items()}
            holds = bool(V.must_drop_holds(B).all())
            assert holds == b["drop_plain"] == (name != "small-2^-6"), name
            d2 = b["rad"][:32] ** 2 + (2.5 * B["W16"] if holds else B["W16"] + B["resid"] + 1.25 * B["E16"])
            assert (d2 > b["rad"][:32] ** 2 + B["W16"] + B["resid"] + B["E16"]).all(), name


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(V.SETS))
def test_keep_words_on_the_shared_sets(name, pt):
    S, R = V.SETS[name], _call(name)
    kept_extra = evals = 0
    for n, b in enumerate(S["blocks"]):
        at = slice(64 * n, 64 * n + 64)
        hit, packed, matrix, exact = R["hit"][at], R["packed"][at], R["matrix"][at], R["exact"][at]
        rays, kind, cen, rad = b["rays"], b["kind"], b["cen"], b["rad"]
        assert (hit == (1 if b["fits"] else 0)).all(), (name, n, "the block's rows fit" if hit.any() else "a row did not fit")
        if not b["fits"]:
            assert np.array_equal(matrix, packed), (name, n, "a block that fell back does not give the packed words")
        finite = np.isfinite(rays).all(axis=1)
        oracle = np.array([[bool(pt.intersect_sphere(rays[i], cen[j], rad[j])[0]) for j in range(64)] for i in range(64)])
        assert np.array_equal(oracle[finite], exact[finite]), (name, n, "the device's exact test and the oracle's disagree")
        assert not exact[~finite].any()
        assert not (exact & ~matrix).any(), (name, n, "the matrix form drops a pair the exact test accepts", np.argwhere(exact & ~matrix)[:4])
        assert not (exact & ~packed).any(), (name, n, "the packed form drops a pair the exact test accepts")
        own = lambda m: m[np.arange(64), b["target"]]   # noqa: E731
        for what in ("hit", "graze", "axis"):
            assert own(exact)[kind == what].all() and own(matrix)[kind == what].all() and own(packed)[kind == what].all(), (name, n, what)
        for what in ("miss", "margin", "nan", "away"):
            assert not own(exact)[kind == what].any(), (name, n, what)
        assert own(matrix)[kind == "inside"].all(), (name, n)
        for what in ("far", "edge"):
            assert matrix[kind == what].all() and packed[kind == what].all(), (name, n, what)
        for what in ("surf_in", "surf_out", "rim"):
            assert not (own(exact) & ~own(matrix))[kind == what].any(), (name, n, what)
        assert np.array_equal(matrix[:, 32:], packed[:, 32:]), (name, n, "the packed loop behind the matrix rows changed its words")
        if b["fits"]:
            assert not own(matrix)[kind == "miss"].any(), (name, n, "an aimed miss beyond W16 + E16 is kept: a row of the A operand is misplaced, or the bound does not hold")
            near = ~np.isin(kind, ("far", "edge", "nan"))
            extra = matrix[near, :32] & ~packed[near, :32] & ~exact[near, :32]
            kept_extra, evals = kept_extra + int(extra.sum()), evals + extra.size
            print("%s block %d: margin rays kept %d of %d" % (name, n, own(matrix)[kind == "margin"].sum(), (kind == "margin").sum()))
    print("%s: exact misses the matrix form keeps and the packed form drops: %d of %d evaluations (%.3f %%)"
          % (name, kept_extra, evals, 100.0 * kept_extra / max(evals, 1)))


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n, S in V.SETS.items() if any(b["fits"] for b in S["blocks"])])
def test_accumulators_on_the_shared_sets(name):
    S, R = V.SETS[name], _call(name)
    worst_t = worst_l = 0.0
    checked = 0
    for n, b in enumerate(S["blocks"]):
        if not b["fits"]:
            continue
        B = b["bounds"]
        for i in range(64):
            ray, s = i % 32, 16 * (i // 32)
            if b["kind"][ray] in ("nan", "far"):
                continue
            o, d = b["rays"][ray, :3] - S["tol"] * b["rays"][ray, 3:], b["rays"][ray, 3:]
            L = b["cen"][s] - o
            tca = float(L @ d)
            tca16, ll16 = R["tuv"][64 * n + i, 0], R["tuv"][64 * n + i, 1]
            assert abs(tca16 - tca) <= B["ET"][s], (name, n, i, tca16, tca)
            target = float(L @ L) - b["rad"][s] ** 2 - B["W16"][s]
            kq = B["kq"][s]
            err = ll16 - target
            assert -B["EL"][s] - B["resid"][s] - 1e-9 * (1 + kq) <= err <= B["EL"][s] + 1e-9 * (1 + kq), (name, n, i, ll16, target)
            worst_t, worst_l = max(worst_t, abs(tca16 - tca) / B["ET"][s]), max(worst_l, abs(err) / B["EL"][s])
            checked += 1
    assert checked >= 64
    print("%s: largest |tca16 - tca'| / ET = %.3f, |ll16 - ll| / EL = %.3f over %d probes" % (name, worst_t, worst_l, checked))

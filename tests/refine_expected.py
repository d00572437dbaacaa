"""The CPU expectation of the pixel refinement (include/rt_hip.h: rt_hip_select_pixels, rt_hip_trace_pixels, rt_hip_blend_pixels):
numpy restatements of the select and of the blend, each next to a scalar loop that says the same one double at a time
(tests/test_refine_cpu.py pins them on each other); the traced entries from the oracle's own trace_sample -- render()'s per-sample
body -- at (x, y, sample_first + k); and the inputs the GPU tests use.
"""
import dataclasses
import math

import numpy as np

import trace_expected as T
from reproject_expected import FLT_MAX, _div, f32, tonemap8  # noqa: F401  (tonemap8: re-exported for the GPU tests)

SEED = 20260404
PIXELS_PER_WORKGROUP = 256   # pt_select_count / pt_select_scatter: a workgroup's pixels
SCAN_PASS = 1024             # pt_select_scan: the counts one workgroup scans; beyond SCAN_PASS workgroups the scan has two levels


# ---- select ----------------------------------------------------------------------------------------------------------------------

def select(values, lo, hi, invert=False):
    """the mask of the selected pixels: (lo <= v && v <= hi) on the exactly widened floats, false for NaN, negated under invert"""
    v = np.asarray(values, dtype=np.float32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        inside = (np.float64(lo) <= v) & (v <= np.float64(hi))
    return ~inside if invert else inside


def select_scalar(values, lo, hi, invert=False):
    out = []
    for v in np.asarray(values, dtype=np.float32).ravel().tolist():   # (tolist widens exactly)
        inside = (lo <= v) and (v <= hi)   # Python's comparisons are IEEE's: false for NaN, -0.0 == 0.0
        out.append((not inside) if invert else inside)
    return np.array(out, dtype=bool).reshape(np.shape(values))


def selected(values, lo, hi, invert=False):
    """-> (indices uint32, ascending; count)"""
    idx = np.flatnonzero(select(values, lo, hi, invert).ravel()).astype(np.uint32)
    return idx, len(idx)


# ---- blend -----------------------------------------------------------------------------------------------------------------------

def blend(pixels, status, radiance, rgb, new_weight, prior_scale, prior=None):
    """rgb: float32 [..., 3] over n_pix pixels (any leading shape).  The entries must name distinct pixels.
    -> dict: rgb (float32, the input's shape), weight (float32 [n_pix]: float(W) at the touched pixels, NaN elsewhere), touched
    (bool [n_pix])"""
    rgb = np.asarray(rgb, dtype=np.float32)
    flat = rgb.reshape(-1, 3).copy()
    n_pix = len(flat)
    pixels = np.asarray(pixels, dtype=np.uint32).astype(np.int64)
    status, r = np.asarray(status).astype(np.int64), np.asarray(radiance, dtype=np.float64).reshape(-1, 3)
    ok = (pixels < n_pix) & (status == 1) & np.isfinite(r).all(axis=1)
    p, r = pixels[ok], r[ok]
    assert len(set(p.tolist())) == len(p), "the restatement is for distinct pixels"
    pr = np.ones(n_pix) if prior is None else np.asarray(prior, dtype=np.float32).astype(np.float64).ravel()
    with np.errstate(all="ignore"):
        wa = np.float64(prior_scale) * pr[p]
        c = flat[p].astype(np.float64)
        replace = ~(wa > 0) | ~np.isfinite(wa) | ~np.isfinite(c).all(axis=1)
        W = np.where(replace, np.float64(new_weight), wa + np.float64(new_weight))
        mixed = (c * wa[:, None] + r * np.float64(new_weight)) / W[:, None]
        out = np.where(replace[:, None], r, mixed).astype(np.float32)
        flat[p] = out
        weight = np.full(n_pix, np.nan, dtype=np.float32)
        weight[p] = W.astype(np.float32)
    touched = np.zeros(n_pix, dtype=bool)
    touched[p] = True
    return dict(rgb=flat.reshape(rgb.shape), weight=weight, touched=touched)


def blend_scalar(pixels, status, radiance, rgb, new_weight, prior_scale, prior=None):
    rgb = np.asarray(rgb, dtype=np.float32)
    flat = rgb.reshape(-1, 3).copy()
    n_pix = len(flat)
    weight, touched = np.full(n_pix, np.nan, dtype=np.float32), np.zeros(n_pix, dtype=bool)
    rad = np.asarray(radiance, dtype=np.float64).reshape(-1, 3)
    for i, p in enumerate(np.asarray(pixels, dtype=np.uint32).tolist()):
        r = [float(x) for x in rad[i]]
        if p >= n_pix or int(status[i]) != 1 or not all(math.isfinite(x) for x in r):
            continue
        wa = float(prior_scale) * (1.0 if prior is None else float(np.asarray(prior, dtype=np.float32).ravel()[p]))
        c = [float(x) for x in flat[p]]
        if not (wa > 0) or not math.isfinite(wa) or not all(math.isfinite(x) for x in c):
            out, W = [f32(x) for x in r], float(new_weight)
        else:
            W = wa + float(new_weight)
            out = [f32(_div(c[k] * wa + r[k] * float(new_weight), W)) for k in range(3)]
        flat[p] = out
        weight[p] = f32(W)
        touched[p] = True
    return dict(rgb=flat.reshape(rgb.shape), weight=weight, touched=touched)


def blend_case(seed, w=19, h=7, n=60):
    """a frame, a prior and a traced list that reach every branch of the blend: priors 0, -0.0, negative, NaN, inf and FLT_MAX
    (a huge finite weight in fp64) and the smallest denormal, a non-finite colour channel, a non-finite radiance channel, status 2, out-of-range
    indices, a radiance beyond float32's range.  -> dict(pixels, status, radiance, rgb, prior)"""
    rng = np.random.default_rng(seed)
    n_pix = w * h
    rgb = rng.uniform(0.0, 2.0, (h, w, 3)).astype(np.float32)
    prior = rng.uniform(0.5, 30.0, (h, w)).astype(np.float32)
    pixels = rng.permutation(n_pix)[:n].astype(np.uint32)
    status = np.ones(n, dtype=np.uint32)
    radiance = rng.uniform(0.0, 3.0, (n, 3))
    planted = [0.0, -0.0, -1.0, np.nan, np.inf, FLT_MAX, 2.0 ** -149]
    for k, v in enumerate(planted):
        prior.ravel()[pixels[k]] = v
    rgb.reshape(-1, 3)[pixels[10], 1] = np.nan
    rgb.reshape(-1, 3)[pixels[11], 0] = np.inf
    rgb.reshape(-1, 3)[pixels[12], 2] = -np.inf
    radiance[20, 0], radiance[21, 1], radiance[22, 2] = np.nan, np.inf, -np.inf
    radiance[23] = (1e300, 1e-300, -0.0)
    status[30], status[31] = 2, 0
    pixels[40], pixels[41] = n_pix, 0xFFFFFFFF
    return dict(pixels=pixels, status=status, radiance=radiance, rgb=rgb, prior=prior)


# ---- trace -----------------------------------------------------------------------------------------------------------------------

def expected_pixels(oracle, sc, pixels, S, s0, seed, casts_oracle=None):
    """oracle: RefOracle / RefMeshOracle at the scene's depth, or PtOracle.  Entry i names pixel pixels[i] of the scene's own frame;
    sample k of a valid entry is oracle.trace_sample(sc, x, y, s0 + k, seed).  -> dict: status uint32 [n] (2 for an index at or
    beyond w * h: zeros), samples [n, S, 3], radiance [n, 3] (trace_expected.reduce_samples: slice = k mod 4), paths / casts uint64
    [n] (casts from casts_oracle, a PtOracle whose ray counter must agree; else tests / primitives)"""
    w, h = sc.width, sc.height
    pixels = np.asarray(pixels, dtype=np.uint32).astype(np.int64).ravel()
    n = len(pixels)
    status, samples = np.ones(n, np.uint32), np.zeros((n, S, 3))
    paths, casts = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    memo = {}
    for i, p in enumerate(pixels.tolist()):
        if p >= w * h:
            status[i] = 2
            continue
        if p not in memo:
            one = (np.zeros((S, 3)), 0, 0)
            for k in range(S):
                rgb, st = oracle.trace_sample(sc, p % w, p // w, s0 + k, seed)
                one[0][k] = rgb
                if casts_oracle is not None:
                    _, st2 = casts_oracle.trace_sample(sc, p % w, p // w, s0 + k, seed, max_depth=sc.max_depth)
                    assert st2["rays"] == st["rays"] and st2["tests"] == st["tests"]
                    c = st2["casts"]
                else:
                    c = st["casts"] if "casts" in st else st["tests"] // sc.n_primitives
                one = (one[0], one[1] + st["rays"], one[2] + c)
            memo[p] = one
        samples[i], paths[i], casts[i] = memo[p]
    return dict(status=status, samples=samples, radiance=T.reduce_samples(samples), paths=paths, casts=casts)


def pixel_list(w, h, seed=SEED):
    """about 40 entries of a w x h frame: the four corners, a duplicate, a descending run, one index = w * h, one = 2^32 - 1, the
    rest scattered"""
    rng = np.random.default_rng(seed)
    n_pix = w * h
    corners = [0, w - 1, (h - 1) * w, n_pix - 1]
    run = list(range(n_pix // 2 + 7, n_pix // 2 - 1, -1))
    rest = rng.choice(n_pix, 24, replace=False).tolist()
    out = corners + [rest[0]] + run + [n_pix] + rest[:12] + [0xFFFFFFFF] + rest[12:]
    return np.array(out, dtype=np.uint32)


# ---- the end-to-end input ------------------------------------------------------------------------------------------------------
# the checkered room (config 4 with M_CHECKERED on the floor's wall sphere) at FULL from LOW: small enough for the CPU, and the
# upsampling with OBJECT_EDGES leaves some pixels, not many, at conf <= 0: the silhouettes, where every tap of the low frame is of
# another object (tests/test_refine_cpu.py checks that on the oracle's buffers; with the default flags no pixel of this frame falls back)
FULL, LOW, SCALE, E2E_SPP, E2E_SEED = (48, 32), (24, 16), 2, 4, 1666943821
E2E_PARAMS = dict(object_edges=True)


def checkered_room(w, h, spp):
    from rt_amd import abi, scene as S
    sc = S.build_scene(4, w, h, spp)
    sc.objects[0].flags |= abi.M_CHECKERED
    return sc


def low_scene(sc, wl, hl):
    """the same objects and camera at another size, as gpu.Preview makes it"""
    return dataclasses.replace(sc, width=wl, height=hl)

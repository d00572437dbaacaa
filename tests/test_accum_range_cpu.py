"""The inputs of tests/test_gpu_accum_range.py and tests/test_gpu_trace_range.py reach what they claim, shown without a GPU:
the kernel the pick table (rt_hip_kernel_for_class) names for every (scene, budget) is the one the GPU test expects; the "flip"
rows change the kernel and the "sum-bound" rows coarsen the fixed-point scale against a 4-sample pass; the hidden emitter's
shell does not leak; and the ray and pixel lists of the trace scenes reach every planted object.
"""
import ctypes as C

import numpy as np
import pytest

import accum_range_scenes as A
import query_expected as Q
import trace_expected as T
import util
from conftest import SEED
from test_views_cpu import scene_class


def _kernel_at(sc, samples):
    from rt_amd import abi
    cls = scene_class(sc, "path", 0)
    cls.samples_per_chunk = samples
    return abi.load_shim().rt_hip_kernel_for_class(C.byref(cls)).decode()


@pytest.mark.parametrize("row", list(A.ACCUM_ROWS))
def test_every_row_names_the_kernel_of_its_budget(row):
    r = A.ACCUM_ROWS[row]
    sc = r["scene"]()
    budget = r["budget"](sc)
    assert 7 < budget <= A.SAMPLES_LIMIT and (budget == 16) == (row in A.SMALL_ROWS)
    at_budget, at_pass = _kernel_at(sc, budget), _kernel_at(sc, 4)
    s_budget, s_pass = util.acc_scale_exp(sc, budget), util.acc_scale_exp(sc, 4)
    print(f"{row}: budget {budget} -> {at_budget} (scale 2^{s_budget}); a pass of 4 -> {at_pass} (2^{s_pass})")
    assert at_budget == r["kernel"]
    if r.get("flip"):
        assert at_pass != at_budget and A.fixed_sums_fit(sc, 4) and not A.fixed_sums_fit(sc, budget)
        assert A.fixed_sums_fit(sc, budget // 2), "the smallest such power of two"
        assert "refr_pool" in at_budget and at_pass == "pt_render_tiles", "windowed by budget, fixed point by pass"
    else:
        assert at_pass == at_budget or r.get("sum_bound")
    if r.get("sum_bound"):
        assert budget > 2 ** 11 and s_budget < s_pass
    else:
        assert s_budget == s_pass, "a budget of 16 keeps the per-term scale"
    if r["kernel"] in ("pt_render_tiles",):
        # the sums stay fixed point: the budget's resolution in a pixel mean must stay below the GPU test's absolute floor
        assert (sc.max_depth + 2) * 2.0 ** (-s_budget - 1) < 1e-9
    sc.free()


def test_budget_that_flips_follows_the_rule_not_a_literal():
    room = A.flip_room()
    b = A.budget_that_flips(room)
    assert b & (b - 1) == 0 and not A.fixed_sums_fit(room, b) and A.fixed_sums_fit(room, b // 2)
    # a brighter light flips earlier, by the rule's own arithmetic: 4 x the emission, a quarter of the budget
    objs, meshes = A._parts(room)
    for o in objs:
        o["emission"] = tuple(4.0 * e for e in o["emission"])
    brighter = A._custom(objs, meshes, 40, 24, 4, 5)
    assert A.budget_that_flips(brighter) == b // 4
    # class_scene()'s own room is too dim to flip within what the shim accepts
    plain = A.LARGEST["scene"]()
    assert A.budget_that_flips(plain) > A.SAMPLES_LIMIT
    print(f"flip budgets: config 4's room 2^{b.bit_length() - 1}, class_scene() 2^{A.budget_that_flips(plain).bit_length() - 1}")


def test_the_largest_budget_row_s_kernel():
    sc = A.LARGEST["scene"]()
    accepted = [b for b in A.largest_candidates() if b <= A.SAMPLES_LIMIT][0]
    assert accepted == A.SAMPLES_LIMIT >= A.LARGEST["at_least"]
    assert _kernel_at(sc, accepted) == A.LARGEST["kernel"] and A.fixed_sums_fit(sc, accepted)
    s = util.acc_scale_exp(sc, accepted)
    assert s < util.acc_scale_exp(sc, 4) and (sc.max_depth + 2) * 2.0 ** (-s - 1) < 1e-9
    sc.free()


@pytest.mark.parametrize("row", [k for k, r in A.ACCUM_ROWS.items() if r.get("hidden")])
def test_the_shell_does_not_leak(pt, row):
    """the oracle's frame with the hidden emitter on equals the frame with it off, at the sizes and sample counts compared"""
    sc = A.ACCUM_ROWS[row]["scene"]()
    dark = A.without_last_emitter(sc)
    for k in (3, 7):
        m1, b1, s1 = pt.render_pixels(sc, SEED, spp=k)
        m0, b0, s0 = pt.render_pixels(dark, SEED, spp=k)
        assert np.array_equal(m1, m0, equal_nan=True) and np.array_equal(b1, b0) and s1 == s0, "the shell leaks: the test's scene is wrong"
    sc.free()
    dark.free()


# ---- trace scenes ----------------------------------------------------------------------------------------------------------------

def _first_hits_of_rays(ref, sc, o, q):
    rays = np.concatenate([o, Q.normalize(o - q)], axis=1)
    exp = Q.expected(ref, sc, rays=rays)
    return np.where(exp["status"] == 1, exp["object"].astype(np.int64), -1)


def pixel_sample_uv(pt, sc, pixels, s, seed):
    """the frame coordinates of sample s of each pixel: render()'s own jitter, the stream's first two draws"""
    w, h = sc.width, sc.height
    uv = np.zeros((len(pixels), 2))
    for i, p in enumerate(np.asarray(pixels).tolist()):
        r = pt.random_doubles(seed, p, s, 2)
        uv[i] = ((p % w + r[0]) / (w - 1.0), (p // w + r[1]) / (h - 1.0))
    return uv


def _check_reach(name, sc, first, hits, samples, paths_per_sample, E, hidden=()):
    """hits [n] (the object the entry's first ray meets), samples [n, S, 3], paths_per_sample [n, S]"""
    kinds = np.array(A.PLANTED)
    for k in range(len(kinds)):
        at = hits == first + k
        if k in hidden:
            assert not at.any(), f"{name}: planted object {k} is in view after all: take it off the list of hidden ones"
            continue
        assert at.any(), f"{name}: no entry's first ray meets planted object {k} ({kinds[k]})"
        if kinds[k] == "zero":
            # prob = 0: the roulette ends every path at its first hit, and the sample is the object's emission (none)
            assert (paths_per_sample[at] == 1).all() and (samples[at] == 0.0).all(), (name, k)
        if kinds[k] == "above_one":
            assert (paths_per_sample[at] > 1).any(), f"{name}: no path bounces off the colour above 1 of object {k}"
        if kinds[k] == "bright":
            assert (samples[at][..., 0] >= 0.5 * E).any(), f"{name}: no sample carries the bright emitter's term"
    neg = np.isin(hits, [first + k for k in range(len(kinds)) if kinds[k] == "negative"])
    assert (samples[neg] < 0).any(), f"{name}: no sample ends below zero"


def _per_sample(oracle, sc, n, sample):
    """-> samples [n, S, 3], paths [n, S] from sample(i, s) -> (rgb, stats)"""
    out, paths = np.zeros((n, A.TRACE_S, 3)), np.zeros((n, A.TRACE_S), np.int64)
    for i in range(n):
        for s in range(A.TRACE_S):
            out[i, s], st = sample(i, s)
            paths[i, s] = st["rays"]
    return out, paths


@pytest.mark.parametrize("name", list(A.TRACE_FORMS))
def test_the_ray_list_reaches_every_planted_object(ref_mesh, name):
    ref = ref_mesh(A.TRACE_DEPTH)
    sc, first = A.trace_range_scene(name, 1e9)
    o, q = A.trace_ray_list(sc, first)
    assert len(o) == 40
    hits = _first_hits_of_rays(ref, sc, o, q)
    width = 2 ** 31 - 1

    def sample(i, s):
        one = T._with_camera(sc, T.ray_camera(o[i], q[i]), width)
        return ref.trace_sample(one, i, 0, s, A.TRACE_SEED)
    samples, paths = _per_sample(ref, sc, len(o), sample)
    _check_reach(name, sc, first, hits, samples, paths, 1e9)
    sc.free()


@pytest.mark.parametrize("name", list(A.TRACE_FORMS))
def test_the_pixel_list_reaches_every_planted_object(ref_mesh, pt, name):
    ref = ref_mesh(A.TRACE_DEPTH)
    sc, first = A.trace_range_scene(name, 1e9)
    pixels = A.trace_pixel_list(sc, first)
    assert len(pixels) == 40 and (pixels < sc.width * sc.height).all()
    # the first ray of sample 0 of every listed pixel
    exp = Q.expected(ref, sc, uv=pixel_sample_uv(pt, sc, pixels, 0, A.TRACE_SEED))
    hits = np.where(exp["status"] == 1, exp["object"].astype(np.int64), -1)
    w = sc.width
    samples, paths = _per_sample(ref, sc, len(pixels), lambda i, s: ref.trace_sample(sc, int(pixels[i]) % w, int(pixels[i]) // w, s, A.TRACE_SEED))
    # (samples 1 .. 4 of a pixel on an object's silhouette may start elsewhere: ask the zero-colour rule of sample 0 alone)
    _check_reach(name, sc, first, hits, samples[:, :1], paths[:, :1], 1e9, hidden=A.MEM_HIDDEN_FROM_CAMERA if name == "mem" else ())
    sc.free()


def test_absolute_emission_keeps_the_paths(ref_mesh):
    """paths depend on colours and the stream, not on emission: the absolute-emission scene traces the same rays, and where no term
    of a sample is negative its value is the sample's own, bit for bit"""
    ref = ref_mesh(A.TRACE_DEPTH)
    sc, first = A.trace_range_scene("plain", 1e30)
    ab, _ = A.trace_range_scene("plain", 1e30, absolute=True)
    o, q = A.trace_ray_list(sc, first)
    a = T.reference_samples(ref, sc, o, q, A.TRACE_S, A.TRACE_SEED)
    b = T.reference_samples(ref, ab, o, q, A.TRACE_S, A.TRACE_SEED)
    assert (a["paths"] == b["paths"]).all() and (a["casts"] == b["casts"]).all()
    assert (b["samples"] >= np.abs(a["samples"])).all()
    mixed = b["samples"] != np.abs(a["samples"])
    assert mixed.any() and not mixed.all()
    sc.free()
    ab.free()

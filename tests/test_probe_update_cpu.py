"""Probe updates without a GPU (include/rt_hip.h, "probe updates"): the numpy and the scalar restatement of tests/probe_update_expected.py
agree bit for bit on random and crafted inputs; the round's probe sequence is the definition's; the blended depth moments keep their
variance non-negative; and the shim refuses bad arguments before it looks for a device."""
import ctypes as C
import itertools

import numpy as np
import pytest

import probe_update_expected as PU


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def _same(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return ((_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))).all()


@pytest.mark.parametrize("n", [1, 17, 18])
@pytest.mark.parametrize("stride", [1, 2, 5, 18, 19])
def test_the_rounds_probes(n, stride):
    seen = []
    for phase in range(stride):
        want = PU.probes_scalar(n, stride, phase)
        got = PU.probes(n, stride, phase)
        assert PU.count(n, stride, phase) == len(want) and list(got) == want
        assert (phase >= n) == (len(want) == 0)
        seen += want
    assert sorted(seen) == list(range(n))   # the phases of a stride cover every probe once


def test_the_shim_counts_the_same():
    from rt_amd import abi
    shim = abi.load_shim()
    for n, stride in itertools.product((1, 17, 18), (1, 2, 5, 18, 19)):
        grid = abi.probe_grid((0, 0, 0), (1, 1, 1), (n, 1, 1))
        for phase in range(stride):
            upd = abi.probe_update(stride, phase)
            assert shim.rt_hip_probe_update_count(C.byref(grid), C.byref(upd)) == PU.count(n, stride, phase)


def test_alpha():
    ages = np.array(list(PU.AGES) + [2, 3, 11, 100], dtype=np.uint32)
    for h in (0.0, 0.5, 0.9, 0.99):
        a = PU.alpha(ages, h)
        assert [float(x) for x in a] == [PU.alpha_scalar(x, h) for x in ages]
        assert a[0] == 1.0 and ((a == 1.0) == ((ages == 0) | (h == 0.0))).all()
    assert PU.alpha_scalar(9, 0.9) == 1.0 / 10.0 and PU.alpha_scalar(10, 0.9) == 1.0 - 0.9   # where the warm-up hands over


def _coeff_case(n, upd, samples, seed):
    age, coeff, _, change = PU.crafted_state(n, 4, seed)
    total = PU.crafted_sums(PU.count(n, upd.stride, upd.phase), samples, seed + 1)
    return age, coeff, change, total


@pytest.mark.parametrize("h", [0.0, 0.9])
@pytest.mark.parametrize("stride,phase", [(1, 0), (4, 1), (19, 3), (70, 69)])
def test_coefficient_blend_numpy_equals_scalar(h, stride, phase):
    n, samples = 67, 8
    for change, fast in ((0.0, 0.0), (0.25, 0.5), (1e-3, 0.0)):
        upd = PU.Update(stride, phase, 0, h, change, fast)
        age, coeff, chg, total = _coeff_case(n, upd, samples, 11)
        out, out_f, out_change = PU.blend_coeff(total, samples, upd, age, coeff, chg)
        idx = PU.probes_scalar(n, stride, phase)
        for j, i in enumerate(idx):
            want, want_change = PU.blend_coeff_scalar(total[j], samples, upd, age[i], coeff[i])
            assert _same(out[i], want), (i, age[i])
            assert _same(out_change[i], want_change)
            if age[i] == 0:   # the NaN the old state holds where the age is 0 does not leak
                assert _same(out[i], (total[j] * (1.0 / samples)) * PU.K[PU.SPHERE]) and out_change[i] == 1.0
        rest = np.setdiff1d(np.arange(n), idx)
        assert _same(out[rest], coeff[rest]) and _same(out_change[rest], chg[rest])
        with np.errstate(all="ignore"):
            assert ((out_f.view(np.uint32) == out.astype(np.float32).view(np.uint32)) | np.isnan(out_f)).all()


def test_the_fast_rule_on_its_threshold():
    """c == change * m keeps the plain alpha, one ulp above takes the fast one: the comparison is a strict >"""
    samples = 8
    upd = PU.Update(1, 0, 0, 0.9, 0.25, 0.5)
    plain = PU.Update(1, 0, 0, 0.9, 0.0, 0.0)
    for old, total, side in PU.threshold_case(upd.change, samples):
        got, _ = PU.blend_coeff_scalar(total, samples, upd, 10, old)
        slow, _ = PU.blend_coeff_scalar(total, samples, plain, 10, old)
        vec, _, _ = PU.blend_coeff(total[None], samples, upd, np.array([10], dtype=np.uint32), old[None])
        assert _same(vec[0], got)
        assert _same(got, slow) == (side <= 0), side


@pytest.mark.parametrize("h", [0.0, 0.9])
@pytest.mark.parametrize("stride,phase", [(1, 0), (4, 1), (70, 69)])
def test_moment_blend_numpy_equals_scalar(h, stride, phase):
    n, texels, d_max = 67, 4, 3.0
    upd = PU.Update(stride, phase, 0, h)
    age, _, moments, _ = PU.crafted_state(n, texels, 21)
    idx = PU.probes_scalar(n, stride, phase)
    sums = PU.crafted_depth_sums(len(idx), texels)
    out = PU.blend_moments(sums, d_max, upd, age, moments)
    for j, i in enumerate(idx):
        for t in range(texels):
            want = PU.blend_moments_scalar(*sums[j, t], d_max, upd, age[i], moments[i, t])
            assert _same(out[i, t], want), (i, t, age[i], sums[j, t])
            if age[i] == 0 and not np.isnan(sums[j, t, 0]):
                assert np.isfinite(out[i, t]).all() or sums[j, t, 0] < 1e-300   # the old NaN does not leak
    rest = np.setdiff1d(np.arange(n), idx)
    assert _same(out[rest], moments[rest])


def test_age_step():
    age = np.array(list(PU.AGES) * 3, dtype=np.uint32)
    for stride, phase in ((1, 0), (4, 3), (19, 0)):
        upd = PU.Update(stride, phase)
        out = PU.age_step(age, upd)
        idx = PU.probes_scalar(len(age), stride, phase)
        for i in range(len(age)):
            assert out[i] == (PU.age_step_scalar(age[i]) if i in idx else age[i])
    assert PU.age_step_scalar(PU.AGE_MAX) == PU.AGE_MAX and PU.age_step_scalar(PU.AGE_MAX - 1) == PU.AGE_MAX


def test_blended_moments_keep_their_variance():
    """Convexity: for finite (mean, mean2) with mean2 >= mean*mean on both sides, the blend (old*keep) + (f*alpha) keeps
    mean2 - mean*mean >= -2^-40 * mean2: in exact arithmetic the blend of two points above the parabola lies above it, and the
    roundings -- two products and an add a moment, a division a fresh moment -- move each by a few 2^-53 of itself."""
    rng = np.random.default_rng(77)
    pairs = 10 ** 4
    mean_o = rng.uniform(0.0, 50.0, pairs)
    old = np.stack([mean_o, mean_o * mean_o + rng.uniform(0.0, 1.0, pairs) * rng.choice([0.0, 1e-9, 1.0], pairs)], axis=-1)
    mean_f = rng.uniform(0.0, 50.0, pairs)
    W = 2.0 ** rng.integers(-8, 4, pairs)   # (powers of two: the fresh moments M / W are the chosen ones exactly)
    m2_f = mean_f * mean_f + rng.uniform(0.0, 1.0, pairs) * rng.choice([0.0, 1e-9, 1.0], pairs)
    old[:, 1] = np.maximum(old[:, 1], old[:, 0] * old[:, 0])
    sums = np.stack([W, W * mean_f, W * np.maximum(m2_f, mean_f * mean_f)], axis=-1)
    f = np.stack([sums[:, 1] / W, sums[:, 2] / W], axis=-1)
    ok = f[:, 1] >= f[:, 0] * f[:, 0]
    assert ok.all() and (old[:, 1] >= old[:, 0] * old[:, 0]).all()   # the premise, on every pair
    ages = rng.choice(np.array(PU.AGES[1:] + (2, 5, 50), dtype=np.int64), pairs).astype(np.uint32)
    for h in (0.5, 0.9, 0.99):
        out = PU.blend_moments(sums[:, None, :], 100.0, PU.Update(1, 0, 0, h), ages, old[:, None, :])[:, 0]
        var = out[:, 1] - out[:, 0] * out[:, 0]
        assert (var[ok] >= -(2.0 ** -40) * out[ok, 1]).all(), var[ok].min()


# ---- refusals need no device -----------------------------------------------------------------------------------------------------------
def _update_call(shim, grid, vis, params, upd, slice_rays=64, ws=256, coeff=256, moments=256, age=256, scene=1):
    """rt_hip_probe_grid_update with made-up addresses: a refusal comes before any of them is used"""
    p = lambda x: None if x is None else C.c_void_p(x)
    return shim.rt_hip_probe_grid_update(p(scene), grid, vis, params, upd, slice_rays, p(ws), p(coeff), None, p(moments), p(age), None, None,
                                         None, None)


def test_refusals_without_a_device():
    from rt_amd import abi
    shim = abi.load_shim()
    EINVAL = -2
    grid = abi.probe_grid((0, 0, 0), (1, 1, 1), (3, 3, 2))
    vis = abi.probe_vis(grid, res=4)
    par = abi.probe_params(abi.PROBE_SPHERE, 8, 1, 4)
    good = dict(stride=1, phase=0, hysteresis=0.9, change=0.0, fast=0.0)
    bad = [dict(stride=0), dict(stride=2, phase=2), dict(stride=1, phase=1), dict(hysteresis=1.0), dict(hysteresis=-0.1),
           dict(hysteresis=float("nan")), dict(hysteresis=float("inf")), dict(fast=1.0), dict(fast=-1e-9), dict(fast=float("nan")),
           dict(change=-1.0), dict(change=float("inf")), dict(change=float("nan"))]
    g, v, q = C.byref(grid), C.byref(vis), C.byref(par)
    for fields in bad:
        upd = abi.probe_update(**{**good, **fields})
        assert _update_call(shim, g, v, q, C.byref(upd)) == EINVAL, fields
        assert shim.rt_hip_probe_age_step(g, C.byref(upd), C.c_void_p(256), None) == EINVAL, fields
        assert shim.rt_hip_probe_blend_coeff(C.c_void_p(256), 8, g, C.byref(upd), C.c_void_p(256), C.c_void_p(256), None, None, None) == EINVAL
        assert shim.rt_hip_probe_blend_moments(C.c_void_p(256), g, v, C.byref(upd), C.c_void_p(256), C.c_void_p(256), None) == EINVAL
        assert shim.rt_hip_probe_update_count(g, C.byref(upd)) == 0
        assert shim.rt_hip_probe_update_workspace_bytes(g, v, C.byref(upd), 64) == 0
        assert shim.rt_hip_probe_grid_update_host(None, 0, None, 0, g, v, q, C.byref(upd), 0, C.c_void_p(256), None, C.c_void_p(256),
                                                  C.c_void_p(256), None, None, None) == EINVAL
    ok = abi.probe_update(**good)
    u = C.byref(ok)
    for field, value in (("struct_size", 40), ("flags", 1), ("reserved", 1)):
        upd = abi.probe_update(**good)
        setattr(upd, field, value)
        assert _update_call(shim, g, v, q, C.byref(upd)) == EINVAL, field
    assert _update_call(shim, g, v, q, None) == EINVAL
    assert _update_call(shim, g, None, q, u) == EINVAL            # moments without a vis
    assert _update_call(shim, g, v, q, u, moments=None) == EINVAL   # a vis without moments
    assert _update_call(shim, g, v, q, u, age=None) == EINVAL
    assert _update_call(shim, g, v, q, u, coeff=None) == EINVAL
    assert _update_call(shim, g, v, q, u, scene=None) == EINVAL
    assert _update_call(shim, g, v, q, u, slice_rays=0) == EINVAL
    assert _update_call(shim, g, v, q, u, ws=264) == EINVAL        # a workspace that is not 16-byte aligned
    # what the two grid bakes refuse
    assert _update_call(shim, None, v, q, u) == EINVAL and _update_call(shim, g, v, None, u) == EINVAL
    hemi = abi.probe_params(abi.PROBE_HEMISPHERE, 8, 1, 4)
    assert _update_call(shim, g, v, C.byref(hemi), u) == EINVAL
    none = abi.probe_params(abi.PROBE_SPHERE, 0, 1, 4)
    assert _update_call(shim, g, v, C.byref(none), u) == EINVAL
    bad_grid = abi.probe_grid((0, 0, 0), (1, 0, 1), (3, 3, 2))
    assert _update_call(shim, C.byref(bad_grid), v, q, u) == EINVAL
    # a finite grid whose last position overflows: a round has no invalid ray because it refuses such a grid
    far_grid = abi.probe_grid((1e308, 0, 0), (1e308, 1, 1), (2, 3, 3))
    assert _update_call(shim, C.byref(far_grid), v, q, u) == EINVAL and b"not finite" in shim.rt_hip_last_error()
    assert shim.rt_hip_probe_grid_update_host(None, 0, None, 0, C.byref(far_grid), v, q, u, 0, C.c_void_p(256), None, C.c_void_p(256),
                                              C.c_void_p(256), None, None, None) == EINVAL
    bad_vis = abi.probe_vis(grid, res=33)
    assert _update_call(shim, g, C.byref(bad_vis), q, u) == EINVAL
    assert shim.rt_hip_probe_blend_coeff(C.c_void_p(256), 0, g, u, C.c_void_p(256), C.c_void_p(256), None, None, None) == EINVAL
    assert shim.rt_hip_probe_blend_moments(C.c_void_p(256), g, v, u, C.c_void_p(256), C.c_void_p(264), None) == EINVAL
    # a round without probes is not an error and needs no device
    far = abi.probe_update(stride=19, phase=18)
    assert _update_call(shim, g, v, q, C.byref(far)) == 0
    assert shim.rt_hip_probe_age_step(g, C.byref(far), C.c_void_p(256), None) == 0
    assert shim.rt_hip_probe_grid_update_host(None, 0, None, 0, g, v, q, C.byref(far), 0, C.c_void_p(256), None, C.c_void_p(256),
                                              C.c_void_p(256), None, None, None) == 0


def test_defaults():
    from rt_amd import abi
    u = abi.probe_update()
    assert (u.struct_size, u.flags, u.stride, u.phase, u.round, u.reserved) == (C.sizeof(abi.RtHipProbeUpdate), 0, 1, 0, 0, 0)
    assert (u.hysteresis, u.change, u.fast) == (0.9, 0.0, 0.0) and C.sizeof(abi.RtHipProbeUpdate) == 48

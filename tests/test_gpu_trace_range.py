"""Radiance queries (pt_trace_rays*) and pixel refinement (pt_trace_pixels*) at the edges of the radiance range: each form's class
scene with a visible emitter of (E, 0.3 E, 1) for E = 1e9 and 1e30, the two negative emitters and the seven edge-colour objects of
accum_range_scenes (tests/test_accum_range_cpu.py shows that the ray and pixel lists reach each of them).  Status, paths and casts
equal the compiled reference; radiance is the stated reduction of the samples; split (and, for pixels, permuted) lists agree bit for
bit; every sample's value meets the project's bar, trace_expected.value_bar -- 2^-40 |ref|, with M_REFRACTION 2^-40 (|ref| + the
entry's largest |ref|).

Samples whose terms cancel.  Where terms of both signs meet, |ref| understates what was summed, and the rounding scales with the
terms, not with their difference.  There the bar is 2^-40 x the same sample of the ABSOLUTE-EMISSION scene (every emission component
replaced by its magnitude, run through the same reference): paths depend on colours and the stream, not on emission -- the test
asserts equal paths and casts of the two reference runs first -- so that value is the sum of |T e|.  Such a sample is recognised by
that value differing from |ref| (a sample whose terms share one sign has the same bits in both runs).

One link to the frame: blend_pixels of the traced radiances equals refine_expected.blend bit for bit, so the values of 1e30 and the
negative ones pass the float32 store and the tonemap bytes.
"""
import numpy as np
import pytest

import accum_range_scenes as A
import refine_expected as R
import trace_expected as T
import upsample_expected as UE

pytestmark = pytest.mark.gpu

ALL_RAYS = ("status", "radiance", "samples", "paths", "casts", "ray")
ALL_PIXELS = ("status", "radiance", "samples", "paths", "casts")
WORST = {}   # (kernel family, form) -> the worst |got - ref| / bar


@pytest.fixture(scope="module")
def gpu():
    import torch
    from rt_amd import abi, gpu as G
    assert abi.load_shim().rt_hip_device_count() >= 1, "no HIP device: the GPU tests must run on the GPU box"
    assert torch.cuda.is_available()
    return G


def _np(out):
    import torch
    torch.cuda.synchronize()
    res = {f: t.cpu().numpy() for f, t in out.items()}
    res["status"] = res["status"].view(np.uint32)
    for f in ("paths", "casts"):
        res[f] = res[f].view(np.uint64)
    return res


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _same(a, b, fields):
    return all((a[f] == b[f]).all() if f in ("status", "paths", "casts") else (_bits(a[f]) == _bits(b[f])).all() for f in fields)


def _stats(a):
    return dict(rays=int(a[0]), casts=int(a[1]), tests=int(a[2]), samples=int(a[3]))


def _check_values(what, key, got, ref, ref_abs, glass):
    """the exact statements and the two value bars -> the worst |got - ref| / bar"""
    assert (ref["paths"] == ref_abs["paths"]).all() and (ref["casts"] == ref_abs["casts"]).all(), f"{what}: emission changed a path"
    assert (got["paths"] == ref["paths"]).all(), f"{what}: paths differ at entries {np.nonzero(got['paths'] != ref['paths'])[0][:5]}"
    assert (got["casts"] == ref["casts"]).all(), f"{what}: casts differ at entries {np.nonzero(got['casts'] != ref['casts'])[0][:5]}"
    assert (_bits(got["radiance"]) == _bits(T.reduce_samples(got["samples"]))).all(), f"{what}: radiance is not the reduction of samples"
    r, a, g = ref["samples"], ref_abs["samples"], got["samples"]
    assert np.array_equal(np.isnan(r), np.isnan(g)) and np.array_equal(np.isposinf(r), np.isposinf(g)) and \
        np.array_equal(np.isneginf(r), np.isneginf(g)), f"{what}: infinite or NaN samples at other places than the reference's"
    fin = np.isfinite(r)
    mixed = fin & (a != np.abs(r))
    assert (a[fin] >= np.abs(r[fin])).all()
    with np.errstate(invalid="ignore"):
        bar = np.where(mixed, T.value_bar(a, glass), T.value_bar(r, glass))
        err = np.abs(g - r)
    ok = fin & (bar > 0)
    ratio = float((err[ok] / bar[ok]).max()) if ok.any() else 0.0
    WORST[key] = max(WORST.get(key, 0.0), ratio)
    print(f"{what}: {int(mixed.sum())} of {int(fin.sum())} sample values have terms of both signs; largest |ref| {float(np.abs(r[fin]).max()):.3e}; "
          f"worst |got - ref| / bar = {ratio:.3e}")
    assert (err[fin] <= bar[fin]).all(), f"{what}: {int((err[fin] > bar[fin]).sum())} sample values beyond the bar, worst ratio {ratio}"
    return mixed


@pytest.mark.parametrize("E", A.TRACE_E, ids=[f"E={e:g}" for e in A.TRACE_E])
@pytest.mark.parametrize("name", list(A.TRACE_FORMS))
def test_rays_at_the_edges_of_the_range(gpu, ref_mesh, pt, name, E):
    form, _, _, glass = A.TRACE_FORMS[name]
    ref_o = ref_mesh(A.TRACE_DEPTH)
    sc, first_obj = A.trace_range_scene(name, E)
    sc_abs, _ = A.trace_range_scene(name, E, absolute=True)
    gs = gpu.GpuScene(sc)
    assert gs.trace_kernel_name() == form
    o, q = A.trace_ray_list(sc, first_obj)
    n, S = len(o), A.TRACE_S
    any_mixed = False
    for first in (0, 3):
        ref = T.reference_samples(ref_o, sc, o, q, S, A.TRACE_SEED, first, casts_oracle=pt)
        ref_abs = T.reference_samples(ref_o, sc_abs, o, q, S, A.TRACE_SEED, first)
        got = _np(gs.trace_rays(ref["rays"], S, A.TRACE_SEED, index_first=first, want=ALL_RAYS))
        assert (got["status"] == 1).all() and (_bits(got["ray"]) == _bits(ref["rays"])).all()
        assert _stats(got["stats"]) == dict(rays=int(ref["paths"].sum()), casts=int(ref["casts"].sum()),
                                            tests=int(ref["casts"].sum()) * sc.n_primitives, samples=n * S)
        any_mixed |= bool(_check_values(f"{form} {name} E={E:g} first={first}", ("rays", name), got, ref, ref_abs, glass).any())
        assert (ref["samples"][..., 0] >= 0.5 * E).any() and (ref["samples"] < 0).any(), "the list should meet the bright and the negative emitters"
        for a, b in ((0, 17), (17, n)):                                                   # the list split under index_first
            part = _np(gs.trace_rays(ref["rays"][a:b], S, A.TRACE_SEED, index_first=first + a, want=ALL_RAYS))
            assert _same(part, {f: got[f][a:b] for f in ALL_RAYS}, ALL_RAYS), f"{name}: split at {a}"
    assert any_mixed, "no sample had terms of both signs: the second bar was never used"
    assert gs.launch_status() == 0
    gs.close()
    for s in (sc, sc_abs):
        s.free()


@pytest.mark.parametrize("E", A.TRACE_E, ids=[f"E={e:g}" for e in A.TRACE_E])
@pytest.mark.parametrize("name", list(A.TRACE_FORMS))
def test_pixels_at_the_edges_of_the_range(gpu, ref_mesh, pt, name, E):
    import torch
    _, form, _, glass = A.TRACE_FORMS[name]
    ref_o = ref_mesh(A.TRACE_DEPTH)
    sc, first_obj = A.trace_range_scene(name, E)
    sc_abs, _ = A.trace_range_scene(name, E, absolute=True)
    gs = gpu.GpuScene(sc)
    assert gs.pixel_kernel_name() == form
    pixels = A.trace_pixel_list(sc, first_obj)
    n, S, w, h = len(pixels), A.TRACE_S, sc.width, sc.height
    any_mixed = False
    for s0 in (0, 3):
        ref = R.expected_pixels(ref_o, sc, pixels, S, s0, A.TRACE_SEED, casts_oracle=pt)
        ref_abs = R.expected_pixels(ref_o, sc_abs, pixels, S, s0, A.TRACE_SEED)
        out = gs.trace_pixels(pixels, S, A.TRACE_SEED, sample_first=s0, want=ALL_PIXELS)
        got = _np(out)
        assert (got["status"] == ref["status"]).all() and (got["status"] == 1).all()
        assert _stats(got["stats"]) == dict(rays=int(ref["paths"].sum()), casts=int(ref["casts"].sum()),
                                            tests=int(ref["casts"].sum()) * sc.n_primitives, samples=n * S)
        any_mixed |= bool(_check_values(f"{form} {name} E={E:g} s0={s0}", ("pixels", name), got, ref, ref_abs, glass).any())
        perm = np.random.default_rng(3).permutation(n)                                    # the list permuted
        moved = _np(gs.trace_pixels(pixels[perm], S, A.TRACE_SEED, sample_first=s0, want=ALL_PIXELS))
        assert _same(moved, {f: got[f][perm] for f in ALL_PIXELS}, ALL_PIXELS), f"{name}: permuted"
        for a, b in ((0, 17), (17, n)):                                                   # ... and split into two calls
            part = _np(gs.trace_pixels(pixels[a:b], S, A.TRACE_SEED, sample_first=s0, want=ALL_PIXELS))
            assert _same(part, {f: got[f][a:b] for f in ALL_PIXELS}, ALL_PIXELS), f"{name}: split at {a}"
        # the link to the frame: the traced radiances blended into a frame (distinct pixels: the first entry of each)
        _, keep = np.unique(pixels, return_index=True)
        keep = np.sort(keep)
        frame = np.random.default_rng(5).uniform(0.0, 2.0, (h, w, 3)).astype(np.float32)
        exp = R.blend(pixels[keep], got["status"][keep], got["radiance"][keep], frame, float(S), 2.0)
        at = torch.from_numpy(keep).cuda()
        rgb, rgb8 = torch.from_numpy(frame.copy()).cuda(), torch.full((h, w, 3), 77, dtype=torch.uint8, device="cuda")
        gpu.blend_pixels(pixels[keep], out["status"][at].contiguous(), out["radiance"][at].contiguous(), rgb, w, h, float(S), 2.0, rgb8=rgb8)
        torch.cuda.synchronize()
        t = exp["touched"]
        assert t.sum() == len(keep) and UE.same_floats(rgb.cpu().numpy(), exp["rgb"]), f"{name}: the blend is not its restatement"
        g8 = rgb8.cpu().numpy().reshape(-1, 3)
        assert (g8[t] == R.tonemap8(exp["rgb"]).reshape(-1, 3)[t]).all() and (g8[~t] == 77).all()
        big = np.abs(exp["rgb"].reshape(-1, 3)[t]).max()
        assert big >= 0.1 * E / (S + 2.0) or name == "mem" and big > 0, "the bright emitter's value should pass the float32 store"
    assert (got["radiance"] < 0).any(), "a negative mean should pass the store too"
    assert any_mixed, "no sample had terms of both signs: the second bar was never used"
    assert gs.launch_status() == 0
    gs.close()
    for s in (sc, sc_abs):
        s.free()


def test_zz_worst_ratios(gpu):
    print("worst |got - ref| / bar per kernel family and form:", {f"{k[0]}:{k[1]}": f"{v:.3e}" for k, v in sorted(WORST.items())})
    assert WORST and all(v <= 1.0 for v in WORST.values())

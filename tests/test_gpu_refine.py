"""Pixel refinement on the GPU (rt_hip_select_pixels, rt_hip_trace_pixels, rt_hip_blend_pixels): the select equals np.flatnonzero of
the restatement around every workgroup, wave and scan-pass edge; the trace gives, on each of its five forms and on a glass scene,
the compiled reference's paths and casts exactly and its sample values to 2^-40, with the contract's three bit-exact properties;
the blend equals its restatement bit for bit; Preview.frame(fill=) and Temporal.frame(fill=) touch exactly the pixels their maps
select and leave every other bit as it is without the argument.

The value bar is the radiance queries' (tests/test_gpu_trace.py, trace_expected.value_bar): 2^-40 |ref|, with M_REFRACTION
2^-40 (|ref| + the entry's largest |ref|)."""
import ctypes as C

import numpy as np
import pytest

import refine_expected as R
import trace_expected as T
import upsample_expected as UE
import util

pytestmark = pytest.mark.gpu

W, H, DEPTH = 31, 23, 4     # the traced frame: ragged against the 8 x 8 tiles, at most 32 x 24
ALL = ("status", "radiance", "samples", "paths", "casts")
SENTINEL = 0x7EADBEEF
COMPARED = set()
_CACHE = {}

# the five forms as tests/test_gpu_trace.py reaches them (trace_expected.SCENES: the same scene classes at this file's frame size),
# and a glass room: name -> (form, scene, glass)
SCENES = {
    "pixels": ("pt_trace_pixels", dict(n_packed=4), False),
    "big": ("pt_trace_pixels_big", dict(n_packed=4, wide=True), False),
    "tri": ("pt_trace_pixels_tri", dict(n_packed=4, tris=40), False),
    "tri_big": ("pt_trace_pixels_tri_big", dict(n_packed=4, tris=400, open_back=True), False),
    "mem": ("pt_trace_pixels_mem", dict(n_packed=249, tris=60), False),
    "glass": ("pt_trace_pixels", dict(n_packed=4, refr=True), True),
}


@pytest.fixture
def gpu():
    import torch
    from rt_amd import abi, gpu as G
    assert abi.load_shim().rt_hip_device_count() >= 1, "no HIP device: the GPU tests must run on the GPU box"
    assert torch.cuda.is_available()
    return G


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def _np(out):
    import torch
    torch.cuda.synchronize()
    res = {f: t.cpu().numpy() for f, t in out.items()}
    res["status"] = res["status"].view(np.uint32)
    for f in ("paths", "casts"):
        if f in res:
            res[f] = res[f].view(np.uint64)
    return res


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _same(a, b, fields=ALL):
    return all((a[f] == b[f]).all() if f in ("status", "paths", "casts") else (_bits(a[f]) == _bits(b[f])).all() for f in fields)


# ---- select ----------------------------------------------------------------------------------------------------------------------

SIZES = [(1, 1), (63, 1), (64, 1), (65, 1), (255, 1), (256, 1), (257, 1), (1, 257), (257, 3), (1, 1000),
         (52429, 5)]    # 262,145 pixels: one past SCAN_PASS x PIXELS_PER_WORKGROUP, so 1,025 counts and a second scan level
assert SIZES[-1][0] * SIZES[-1][1] == R.SCAN_PASS * R.PIXELS_PER_WORKGROUP + 1


def _select(G, values, w, h, lo, hi, invert=False, capacity=None):
    """-> (the indices buffer as uint32, prefilled with SENTINEL; count)"""
    import torch
    cap = w * h if capacity is None else capacity
    buf = torch.full((max(cap, 1),), SENTINEL, dtype=torch.int32, device="cuda") if cap else None
    idx, count = G.select_pixels(_dev(values), w, h, lo, hi, invert=invert, capacity=cap, indices=buf)
    torch.cuda.synchronize()
    return (idx.cpu().numpy().view(np.uint32)[:cap] if cap else None), count


def _check_select(G, values, w, h, lo, hi, invert=False, capacity=None):
    want, n = R.selected(values, lo, hi, invert)
    got, count = _select(G, values, w, h, lo, hi, invert, capacity)
    what = (w, h, lo, hi, invert, capacity)
    assert count == n, what
    if got is not None:
        k = min(n, len(got))
        assert (got[:k] == want[:k]).all(), what
        assert (got[k:] == SENTINEL).all(), what     # the tail is left untouched
    return n


@pytest.mark.parametrize("w,h", SIZES, ids=lambda v: str(v))
def test_select_equals_flatnonzero(gpu, w, h):
    n = w * h
    rng = np.random.default_rng(n)
    values = rng.uniform(-1.0, 2.0, n).astype(np.float32)
    special = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1.0, 2.0 ** -149], dtype=np.float32)
    at = rng.permutation(n)[:min(n, len(special))]
    values[at] = special[:len(at)]
    if n > 64:
        values[63], values[64], values[n - 1] = 0.5, np.nan, 0.0     # a wave's last lane, the next wave's first, the last pixel
    counts = set()
    for lo, hi, invert in [(0.0, 1.0, False), (0.0, 1.0, True), (-np.inf, 0.0, False), (-np.inf, np.inf, False), (-np.inf, np.inf, True),
                           (1.0, 0.0, False), (1.0, 0.0, True), (-0.0, 0.0, False), (np.inf, np.inf, False)]:
        counts.add(_check_select(gpu, values, w, h, lo, hi, invert))
    assert n in counts                                                    # lo > hi under INVERT selects everything, NaN included
    assert _check_select(gpu, np.full(n, 3.0, np.float32), w, h, 0.0, 1.0) == 0          # none selected
    assert _check_select(gpu, np.full(n, 0.5, np.float32), w, h, 0.0, 1.0) == n          # all selected
    every = np.full(n, 3.0, np.float32)
    every[::64] = 0.25
    assert _check_select(gpu, every, w, h, 0.0, 1.0) == (n + 63) // 64                   # every 64th pixel
    full = _check_select(gpu, values, w, h, 0.0, 1.0, capacity=0)                        # count only, no indices
    if full > 1:
        assert _check_select(gpu, values, w, h, 0.0, 1.0, capacity=full // 2) == full     # capacity below the count: the count is full
        assert _check_select(gpu, values, w, h, 0.0, 1.0, capacity=full - 1) == full


# ---- trace -----------------------------------------------------------------------------------------------------------------------

def _scene(G, name):
    if name not in _CACHE:
        sc = util.class_scene(depth=DEPTH, width=W, height=H, **SCENES[name][1])
        _CACHE[name] = (sc, G.GpuScene(sc))
    return _CACHE[name]


def _stats(a):
    return dict(rays=int(a[0]), casts=int(a[1]), tests=int(a[2]), samples=int(a[3]))


@pytest.mark.parametrize("name", list(SCENES))
def test_trace_equals_the_reference(gpu, ref_mesh, pt, name):
    """S = 5 at sample_first 0 and 3 over refine_expected.pixel_list: status, paths and casts exactly, every sample inside the bar,
    (a) the reduction, (b) permuted and split lists, (c) a sample is a function of (p, s) -- all bit for bit"""
    form, _, glass = SCENES[name]
    sc, gs = _scene(gpu, name)
    assert gs.pixel_kernel_name() == form
    pixels = R.pixel_list(W, H)
    assert 36 <= len(pixels) <= 44
    valid = pixels < W * H
    got_at = {}
    for s0 in (0, 3):
        ref = R.expected_pixels(ref_mesh(DEPTH), sc, pixels, 5, s0, R.SEED, casts_oracle=pt)
        got = _np(gs.trace_pixels(pixels, 5, R.SEED, sample_first=s0, want=ALL))
        got_at[s0] = got
        assert (got["status"] == ref["status"]).all() and got["status"].tolist().count(2) == 2
        for f in ("radiance", "samples", "paths", "casts"):
            assert (got[f][~valid] == 0).all(), f
        assert (got["paths"] == ref["paths"]).all(), f"{name}: paths differ at entries {np.nonzero(got['paths'] != ref['paths'])[0][:5]}"
        assert (got["casts"] == ref["casts"]).all(), f"{name}: casts differ at entries {np.nonzero(got['casts'] != ref['casts'])[0][:5]}"
        st = _stats(got["stats"])
        assert st == dict(rays=int(ref["paths"].sum()), casts=int(ref["casts"].sum()), tests=int(ref["casts"].sum()) * sc.n_primitives,
                          samples=int(valid.sum()) * 5), (name, st)
        err, bar = np.abs(got["samples"] - ref["samples"]), T.value_bar(ref["samples"], glass)
        ratio = float((err[bar > 0] / bar[bar > 0]).max())
        print(f"{name} s0={s0}: worst |got - ref| / bar = {ratio:.3e}")
        assert (err <= bar).all(), f"{name}: {(err > bar).sum()} sample values beyond the bar, worst ratio {ratio}"
        assert (_bits(got["radiance"]) == _bits(T.reduce_samples(got["samples"]))).all(), f"{name}: (a) radiance is not the reduction"
    whole = got_at[3]
    dup = np.flatnonzero(pixels == pixels[4])
    assert len(dup) == 2 and all((_bits(whole[f][dup[0]]) == _bits(whole[f][dup[1]])).all() for f in ("radiance", "samples"))
    perm = np.random.default_rng(3).permutation(len(pixels))                              # (b) the list permuted
    moved = _np(gs.trace_pixels(pixels[perm], 5, R.SEED, sample_first=3, want=ALL))
    assert _same({f: moved[f] for f in ALL}, {f: whole[f][perm] for f in ALL}), f"{name}: (b) permuted"
    for a, b in ((0, 17), (17, len(pixels))):                                             # (b) split into two calls
        part = _np(gs.trace_pixels(pixels[a:b], 5, R.SEED, sample_first=3, want=ALL))
        assert _same(part, {f: whole[f][a:b] for f in ALL}), f"{name}: (b) split at {a}"
    eight = _np(gs.trace_pixels(pixels, 8, R.SEED, sample_first=0, want=("status", "samples")))   # (c)
    four = _np(gs.trace_pixels(pixels, 4, R.SEED, sample_first=4, want=("status", "samples")))
    assert (_bits(eight["samples"][:, 4:]) == _bits(four["samples"])).all(), f"{name}: (c) samples 4 .. 7"
    assert (_bits(eight["samples"][:, :5]) == _bits(got_at[0]["samples"])).all(), f"{name}: (c) samples do not depend on S"
    assert (_bits(eight["samples"][:, 3:]) == _bits(got_at[3]["samples"])).all()
    assert gs.launch_status() == 0
    COMPARED.add(form)


def test_trace_call_forms(gpu):
    import torch
    from rt_amd import abi
    shim = abi.load_shim()
    sc, gs = _scene(gpu, "pixels")
    before = [C.c_uint64(0) for _ in range(shim.rt_hip_pixel_kernel_count())]
    for k, c in enumerate(before):
        shim.rt_hip_pixel_kernel_launches(k, C.byref(c))
    out = gs.trace_pixels(np.zeros(0, np.uint32), 3, R.SEED, want=ALL)                    # n == 0 launches nothing
    torch.cuda.synchronize()
    assert out["status"].numel() == 0 and (out["stats"] == 0).all()
    for k, c in enumerate(before):
        now = C.c_uint64(0)
        shim.rt_hip_pixel_kernel_launches(k, C.byref(now))
        assert now.value == c.value
    pixels = R.pixel_list(W, H)
    dev = _np(gs.trace_pixels(pixels, 5, R.SEED, sample_first=3, want=ALL))
    d_pix = _dev(pixels)
    for kw in (dict(samples=0), dict(sample_first=-1), dict(samples=2 ** 30, sample_first=2 ** 30 + 1), dict(integrator=abi.CAST_RAY),
               dict(width=1), dict(max_depth=-1)):
        p = abi.pixel_params(W, H, 5, R.SEED)
        for f, v in kw.items():
            setattr(p, f, v)
        rad = abi.RtHipRadiance()
        rad.status = torch.zeros(len(pixels), dtype=torch.int32, device="cuda").data_ptr()
        assert shim.rt_hip_trace_pixels(gs.handle, C.byref(sc.camera), C.c_void_p(d_pix.data_ptr()), len(pixels), C.byref(p), C.byref(rad),
                                        None, None) == abi.EINVAL, kw
    with pytest.raises(gpu.ShimError):
        gs.trace_pixels(pixels, 5, R.SEED, max_depth=1000001)
    glass_sc, glass_gs = _scene(gpu, "glass")
    with pytest.raises(gpu.ShimError):                                                       # RT_HIP_ELIMIT with M_REFRACTION
        glass_gs.trace_pixels(pixels, 1, R.SEED, max_depth=33)
    assert shim.rt_hip_set_device_map((C.c_int * 3)(0, 0, 0), 3) == 0                       # the host form on a logical device
    try:
        host = gpu.trace_pixels_host(sc, pixels, 5, R.SEED, sample_first=3, device=2, want=ALL)
        with pytest.raises(gpu.ShimError):
            gpu.trace_pixels_host(sc, pixels[:4], 5, R.SEED, device=3)
    finally:
        assert shim.rt_hip_set_device_map(None, 0) == 0
    assert _same(host, dev)
    assert host["stats"]["rays"] == int(dev["paths"].sum())
    assert gs.launch_status() == 0


def test_trace_against_the_rendered_frame(gpu):
    """the sanity link to the frame: float(radiance) at S = 16, sample_first = 0 of every pixel against rt_hip_render_tiles' 16-spp
    frame, within the project's image bar (1e-4 RMS per channel).  Not asserted tighter: the frame comes from the pooled body, whose
    fixed-point sum is another reduction than the four slice sums.  The worst per-channel difference in float32 ulps is printed"""
    sc, gs = _scene(gpu, "pixels")
    img, _, st = gs.render_image(R.SEED, 16)
    frame = img.cpu().numpy().reshape(-1, 3)
    out = _np(gs.trace_pixels(np.arange(W * H, dtype=np.uint32), 16, R.SEED, want=("status", "radiance")))
    assert (out["status"] == 1).all()
    mine = out["radiance"].astype(np.float32)
    rms = util.channel_rms(mine.astype(np.float64), frame.astype(np.float64))
    ulps = np.abs(mine.view(np.int32).astype(np.int64) - frame.view(np.int32).astype(np.int64))
    ts = _stats(out["stats"])
    print(f"\n{gs.last_launch_kernel()} against {gs.pixel_kernel_name()}: RMS {np.max(rms):.3e}, worst difference {int(ulps.max())} float32 ulps, "
          f"{int((ulps > 0).sum())} of {ulps.size} channels differ")
    assert (np.asarray(rms) <= util.RMS_TOL).all()
    assert (ts["rays"], ts["casts"], ts["samples"]) == (st["rays"], st["casts"], W * H * 16)     # the same paths, to the last scan


# ---- blend -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nw,ps,with_prior", [(4.0, 0.0, True), (4.0, 4.0, True), (16.0, 1.0, False), (1.0, 2.0 ** 100, True),
                                              (3.0, float("inf"), True), (2.0, 0.0, False)])
def test_blend_equals_the_restatement(gpu, nw, ps, with_prior):
    import torch
    case = R.blend_case(int(nw * 10 + with_prior))
    h, w = case["rgb"].shape[:2]
    prior = case["prior"] if with_prior else None
    exp = R.blend(case["pixels"], case["status"], case["radiance"], case["rgb"], nw, ps, prior)
    t = exp["touched"]
    assert t.sum() == len(case["pixels"]) - 7
    rgb, rgb8, weight = _dev(case["rgb"]), torch.full((h, w, 3), 77, dtype=torch.uint8, device="cuda"), torch.full((h, w), -5.0, device="cuda")
    gpu.blend_pixels(case["pixels"], _dev(case["status"]), _dev(case["radiance"]), rgb, w, h, nw, ps,
                     prior=_dev(prior) if with_prior else None, rgb8=rgb8, weight=weight)
    torch.cuda.synchronize()
    assert UE.same_floats(rgb.cpu().numpy(), exp["rgb"])                               # untouched pixels included: their input bits
    g8, gw = rgb8.cpu().numpy().reshape(-1, 3), weight.cpu().numpy().ravel()
    assert (g8[~t] == 77).all() and (gw[~t] == -5.0).all()                             # bytes and weight only where touched
    assert (g8[t] == R.tonemap8(exp["rgb"]).reshape(-1, 3)[t]).all()
    assert UE.same_floats(gw[t], exp["weight"][t])
    # without the optional outputs, and the weight written over the prior itself
    if with_prior:
        rgb2, pr = _dev(case["rgb"]), _dev(prior)
        gpu.blend_pixels(case["pixels"], _dev(case["status"]), _dev(case["radiance"]), rgb2, w, h, nw, ps, prior=pr, weight=pr)
        torch.cuda.synchronize()
        assert UE.same_floats(rgb2.cpu().numpy(), exp["rgb"])
        assert UE.same_floats(pr.cpu().numpy().ravel()[t], exp["weight"][t]) and UE.same_floats(pr.cpu().numpy().ravel()[~t], prior.ravel()[~t])
    rgb3 = _dev(case["rgb"])
    gpu.blend_pixels(case["pixels"], _dev(case["status"]), _dev(case["radiance"]), rgb3, w, h, nw, ps, n=0)     # n == 0: nothing
    torch.cuda.synchronize()
    assert UE.same_floats(rgb3.cpu().numpy(), case["rgb"])


# ---- end to end -------------------------------------------------------------------------------------------------------------------

def test_preview_fill_touches_exactly_the_fallback_pixels(gpu):
    import torch
    (w, h) = R.FULL
    sc = R.checkered_room(w, h, R.E2E_SPP)
    gs = gpu.GpuScene(sc)
    pv = gs.preview(R.SCALE, **R.E2E_PARAMS)
    assert (pv.low_width, pv.low_height) == R.LOW
    base = pv.frame(R.E2E_SEED, R.E2E_SPP)
    torch.cuda.synchronize()
    assert "filled" not in base
    b_rgb, b_rgb8, conf = base["rgb"].cpu().numpy(), base["rgb8"].cpu().numpy(), base["conf"].cpu().numpy()
    again = pv.frame(R.E2E_SEED, R.E2E_SPP, fill=None)
    torch.cuda.synchronize()
    assert UE.same_floats(again["rgb"].cpu().numpy(), b_rgb) and (again["rgb8"].cpu().numpy() == b_rgb8).all()
    idx, count = R.selected(conf, -np.inf, 0.0)
    assert 1 <= count <= w * h // 4, count                                              # the input tests/test_refine_cpu.py checked
    res = pv.frame(R.E2E_SEED, R.E2E_SPP, fill=4)
    torch.cuda.synchronize()
    assert res["filled"] == count
    assert UE.same_bits(res["conf"].cpu().numpy(), conf)
    rgb, rgb8 = res["rgb"].cpu().numpy().reshape(-1, 3), res["rgb8"].cpu().numpy().reshape(-1, 3)
    rest = np.ones(w * h, bool)
    rest[idx] = False
    assert UE.same_floats(rgb[rest], b_rgb.reshape(-1, 3)[rest]) and (rgb8[rest] == b_rgb8.reshape(-1, 3)[rest]).all()
    traced = _np(gs.trace_pixels(idx, 4, R.E2E_SEED, sample_first=0, want=("status", "radiance")))
    assert (traced["status"] == 1).all()
    want = traced["radiance"].astype(np.float32)
    assert UE.same_floats(rgb[idx], want) and (rgb8[idx] == R.tonemap8(want)).all()
    assert not UE.same_floats(rgb[idx], b_rgb.reshape(-1, 3)[idx])
    assert gs.launch_status() == 0
    pv.close()
    gs.close()
    sc.free()


def test_temporal_fill_touches_exactly_the_short_histories(gpu):
    import torch
    from rt_amd import scene as S
    w, h, spp, fill = 48, 32, 4, 8
    sc = S.build_scene(4, w, h, spp)
    gs = gpu.GpuScene(sc)
    cams = S.orbit_cameras(4, w, h)[-2:]
    plain = gs.temporal()
    for k, cam in enumerate(cams):
        base = plain.frame(cam, R.E2E_SEED + k, spp)
    torch.cuda.synchronize()
    assert "filled" not in base
    b_rgb, b_len, b_rgb8 = base["rgb"].cpu().numpy().reshape(-1, 3), base["len"].cpu().numpy().ravel(), base["rgb8"].cpu().numpy().reshape(-1, 3)
    idx, count = R.selected(b_len, 0.0, 1.0)
    assert 1 <= count < w * h, count                                                    # the move disoccludes some pixels, not all
    filled = gs.temporal()
    filled.frame(cams[0], R.E2E_SEED, spp, fill=None)
    res = filled.frame(cams[1], R.E2E_SEED + 1, spp, fill=fill)
    torch.cuda.synchronize()
    assert res["filled"] == count
    rgb, ln, rgb8 = res["rgb"].cpu().numpy().reshape(-1, 3), res["len"].cpu().numpy().ravel(), res["rgb8"].cpu().numpy().reshape(-1, 3)
    rest = np.ones(w * h, bool)
    rest[idx] = False
    assert UE.same_floats(rgb[rest], b_rgb[rest]) and UE.same_bits(ln[rest], b_len[rest]) and (rgb8[rest] == b_rgb8[rest]).all()
    traced = _np(gs.trace_pixels(idx, fill, R.E2E_SEED + 1, sample_first=spp, camera=cams[1], want=("status", "radiance")))
    exp = R.blend(idx, traced["status"], traced["radiance"], b_rgb, float(fill), float(spp), prior=b_len)
    assert exp["touched"][idx].all()
    assert UE.same_floats(rgb, exp["rgb"]) and (rgb8[idx] == R.tonemap8(exp["rgb"][idx])).all()
    # len rises by fill / spp: (len * spp + fill) rounded to float32, divided by spp in float32
    want_len = exp["weight"][idx] / np.float32(spp)
    assert UE.same_bits(ln[idx], want_len)
    ones = b_len[idx] == 1.0
    assert ones.any() and (ln[idx][ones] == np.float32(1.0 + fill / spp)).all()
    assert gs.launch_status() == 0
    gs.close()
    sc.free()


def test_zz_every_pixel_form_was_compared(gpu):
    from rt_amd import abi
    shim = abi.load_shim()
    for k in range(shim.rt_hip_pixel_kernel_count()):
        n = C.c_uint64(0)
        name = shim.rt_hip_pixel_kernel_launches(k, C.byref(n)).decode()
        assert n.value > 0 and name in COMPARED, f"{name}: {n.value} launches, compared: {name in COMPARED}"
    for sc, gs in _CACHE.values():
        gs.close()
        sc.free()
    _CACHE.clear()

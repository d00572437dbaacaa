"""The ten path-tracing query kernels -- pt_trace_rays[_big|_tri|_tri_big|_mem] and pt_trace_pixels[_big|_tri|_tri_big|_mem] -- under
other cameras, and with their scene far out or scaled (util.VARIANTS), with every material on every form.

These kernels are compiled functions of their own, every one instantiated <REFRACT = true, CHECKER = true>; tests/test_gpu_trace.py
and tests/test_gpu_refine.py compare them from the class's own camera, (0, 0, 50) looking at the origin, and only the first forms
with glass or a checker.  Here each class of trace_view_scenes.TRACE_VIEW_CLASSES (which material meets which form: that module's
table) is traced at 31 x 23, depth 4, through the inside, steep, telephoto, wide, sheared and near_plane cameras and with its scene
moved 2e7 out or scaled by 1e-3 and 1e3:

  1. pixels: trace_pixels over refine_expected.pixel_list at S = 5, sample_first = 3 against the compiled reference's own samples:
     status, paths, casts and the launch's counters exactly, every sample inside trace_expected.value_bar, radiance the reduction
     of the samples bit for bit, the two invalid entries zeros with status 2;
  2. rays: trace_rays over trace_view_scenes.ray_list (camera rays of the variant's camera, the ray set, aimed rays) at S = 3, the
     same comparisons, `ray` bit for bit what was given; the same under origin_radius = the farthest origin (a hint: no output bit
     may change); trace_uv's rays are query_uv's and the reference's get_camera_ray bit for bit, and its samples those of the same
     rays given explicitly;
  3. the call's camera is what counts: on a scene built with the class's own camera, trace_pixels(camera = the variant's) is the
     result of the scene built under the variant, bit for bit, also after a launch with another camera in between (pixels_launch
     acquires a table set per near_R);
  4. last, the tally: each of the ten kernels compared under at least 8 of the 9 variants, every class under all 9; the table of
     forms and of the worst |got - ref| / bar per case is printed (profiles/r12_trace_views.txt is that print).

tests/test_trace_views_cpu.py shows what the lists reach.  The bar is trace_expected.value_bar as it stands (derivation:
tests/test_gpu_trace.py): 2^-40 |ref|, with M_REFRACTION 2^-40 (|ref| + the entry's largest |ref|).  The worst ratios measured
never feed it.
"""
import ctypes as C
import time

import numpy as np
import pytest

import refine_expected as R
import trace_expected as T
import trace_view_scenes as V
from util import VARIANTS, VIEWS

pytestmark = pytest.mark.gpu

PIXEL_FIELDS = ("status", "radiance", "samples", "paths", "casts")
RAY_FIELDS = PIXEL_FIELDS + ("ray",)
RECORD = {}      # (class, variant) -> dict(trace, pixel: the forms compared; rays, pixels: worst |got - ref| / bar)
_PIXELS = {}     # (class, variant) -> trace_pixels' result of the scene built under the variant (None: the class's own)
T0 = [None]


@pytest.fixture(scope="module")
def gpu():
    import torch
    from rt_amd import abi, gpu as G
    assert abi.load_shim().rt_hip_device_count() >= 1, "no HIP device: the GPU tests must run on the GPU box"
    assert torch.cuda.is_available()
    T0[0] = T0[0] or time.time()
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
    return [f for f in fields if not ((a[f] == b[f]).all() if f in ("status", "paths", "casts") else (_bits(a[f]) == _bits(b[f])).all())]


def _stats(a):
    return dict(rays=int(a[0]), casts=int(a[1]), tests=int(a[2]), samples=int(a[3]))


def _launches(kind, form):
    from rt_amd import abi
    shim = abi.load_shim()
    count, fn = ((shim.rt_hip_trace_kernel_count, shim.rt_hip_trace_kernel_launches) if kind == "trace" else
                 (shim.rt_hip_pixel_kernel_count, shim.rt_hip_pixel_kernel_launches))
    for k in range(count()):
        n = C.c_uint64(0)
        if fn(k, C.byref(n)).decode() == form:
            return n.value
    raise KeyError(form)


def _compare(what, sc, got, ref, valid, S, glass):
    """-> the worst |got - ref| / bar.  valid: which entries the contract traces"""
    assert (got["status"] == np.where(valid, 1, 2)).all(), what
    for f in ("radiance", "samples", "paths", "casts"):
        assert (got[f][~valid] == 0).all(), (what, f)
    assert (got["paths"] == ref["paths"]).all(), f"{what}: paths differ at entries {np.nonzero(got['paths'] != ref['paths'])[0][:5]}"
    assert (got["casts"] == ref["casts"]).all(), f"{what}: casts differ at entries {np.nonzero(got['casts'] != ref['casts'])[0][:5]}"
    st = _stats(got["stats"])
    assert st == dict(rays=int(ref["paths"].sum()), casts=int(ref["casts"].sum()), tests=int(ref["casts"].sum()) * sc.n_primitives,
                      samples=int(valid.sum()) * S), (what, st)
    err, bar = np.abs(got["samples"] - ref["samples"]), T.value_bar(ref["samples"], glass)
    ratio = float((err[bar > 0] / bar[bar > 0]).max()) if (bar > 0).any() else 0.0
    print(f"{what}: worst |got - ref| / bar = {ratio:.3e}")
    assert (err <= bar).all(), f"{what}: {(err > bar).sum()} sample values beyond the bar, worst ratio {ratio}"
    assert (_bits(got["radiance"]) == _bits(T.reduce_samples(got["samples"]))).all(), f"{what}: radiance is not the reduction"
    return ratio


def _pixels_under(G, name, variant):
    """trace_pixels of the scene BUILT under the variant, with its own camera (computed once)"""
    if (name, variant) not in _PIXELS:
        sc = V.scene_under(name, variant)
        gs = G.GpuScene(sc)
        _PIXELS[(name, variant)] = _np(gs.trace_pixels(V.pixel_list(), V.PIXEL_S, V.SEED, sample_first=V.PIXEL_S0, want=PIXEL_FIELDS))
        assert gs.launch_status() == 0
        gs.close()
        sc.free()
    return _PIXELS[(name, variant)]


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", V.CLASS_NAMES)
def test_every_form_equals_the_reference_under_every_variant(gpu, ref_mesh, pt, name, variant):
    import torch
    glass = V.CLASSES[name][4]
    tf, pf = V.forms_under(name, variant)
    ref_o = ref_mesh(V.DEPTH)
    sc = V.scene_under(name, variant)
    gs = gpu.GpuScene(sc)
    assert (gs.trace_kernel_name(), gs.pixel_kernel_name()) == (tf, pf), \
        f"{name} {variant}: the scene takes {gs.trace_kernel_name()} / {gs.pixel_kernel_name()}, TRACE_MOVES says {tf} / {pf}"
    what = f"{name} {variant}"

    # 1. pixels
    pixels = V.pixel_list()
    valid = pixels < V.W * V.H
    ref = R.expected_pixels(ref_o, sc, pixels, V.PIXEL_S, V.PIXEL_S0, V.SEED, casts_oracle=pt)
    before = _launches("pixel", pf)
    got = _np(gs.trace_pixels(pixels, V.PIXEL_S, V.SEED, sample_first=V.PIXEL_S0, want=PIXEL_FIELDS))
    assert _launches("pixel", pf) == before + 1, what
    assert got["status"].tolist().count(2) == 2
    worst_p = _compare(f"{what} {pf}", sc, got, ref, valid, V.PIXEL_S, glass)
    assert gs.launch_status() == 0
    _PIXELS.setdefault((name, variant), {f: got[f] for f in PIXEL_FIELDS + ("stats",)})

    # 2. rays
    o, q = V.ray_list(sc, name, variant)
    n = len(o)
    ref = T.reference_samples(ref_o, sc, o, q, V.RAY_S, V.SEED, casts_oracle=pt)
    before = _launches("trace", tf)
    got = _np(gs.trace_rays(ref["rays"], V.RAY_S, V.SEED, want=RAY_FIELDS))
    assert _launches("trace", tf) == before + 1, what
    worst_r = _compare(f"{what} {tf}", sc, got, ref, np.ones(n, bool), V.RAY_S, glass)
    assert (_bits(got["ray"]) == _bits(ref["rays"])).all(), what
    assert gs.launch_status() == 0
    far_out = float(np.sqrt((o * o).sum(axis=1)).max())                       # another near_R, another table set: not a bit moves
    hinted = _np(gs.trace_rays(ref["rays"], V.RAY_S, V.SEED, origin_radius=far_out, want=RAY_FIELDS))
    assert not _same(hinted, got, RAY_FIELDS + ("stats",)), f"{what}: origin_radius = {far_out} changes {_same(hinted, got, RAY_FIELDS)}"
    # the camera rays through the kernel's own load_camera
    uv = V.uv_points()
    by_uv = _np(gs.trace_uv(uv, V.RAY_S, V.SEED, want=RAY_FIELDS))
    q_ray = gs.query_uv(uv, want=("ray",))["ray"]
    torch.cuda.synchronize()
    assert (_bits(by_uv["ray"]) == _bits(q_ray.cpu().numpy())).all(), f"{what}: trace_uv's rays are not query_uv's"
    cam_rays = np.array([ref_o.camera_ray(sc.camera, float(u), float(v)) for u, v in uv])
    assert (_bits(by_uv["ray"]) == _bits(cam_rays)).all(), f"{what}: trace_uv's rays are not get_camera_ray's"
    assert (by_uv["status"] == 1).all()
    given = _np(gs.trace_rays(by_uv["ray"], V.RAY_S, V.SEED, want=RAY_FIELDS))
    assert not _same(given, by_uv, RAY_FIELDS + ("stats",)), f"{what}: the camera rays given explicitly differ in {_same(given, by_uv, RAY_FIELDS)}"
    assert gs.launch_status() == 0
    RECORD[(name, variant)] = dict(trace=tf, pixel=pf, rays=worst_r, pixels=worst_p)
    gs.close()
    sc.free()


@pytest.mark.parametrize("variant", VIEWS)
@pytest.mark.parametrize("name", ["all_sph", "tri_chk", "tri_big_chk"])
def test_the_call_s_camera_is_what_counts(gpu, name, variant):
    """pixels_launch takes near_R from the call's camera and acquires a table set for it: variant camera, the scene's own, the
    variant's again on ONE scene built with the class's own camera (the geometry of a camera variant is the class's, bit for bit)"""
    want = _pixels_under(gpu, name, variant)
    own = _pixels_under(gpu, name, None)
    vsc = V.scene_under(name, variant)
    sc = V.scene_under(name)
    gs = gpu.GpuScene(sc)
    args = (V.pixel_list(), V.PIXEL_S, V.SEED)
    first = _np(gs.trace_pixels(*args, sample_first=V.PIXEL_S0, camera=vsc.camera, want=PIXEL_FIELDS))
    second = _np(gs.trace_pixels(*args, sample_first=V.PIXEL_S0, camera=sc.camera, want=PIXEL_FIELDS))
    third = _np(gs.trace_pixels(*args, sample_first=V.PIXEL_S0, camera=vsc.camera, want=PIXEL_FIELDS))
    fields = PIXEL_FIELDS + ("stats",)
    assert not _same(first, want, fields), f"{name} {variant}: camera= differs from the scene built under it in {_same(first, want, fields)}"
    assert not _same(third, first, fields), f"{name} {variant}: the third launch differs in {_same(third, first, fields)}"
    assert not _same(second, own, fields), f"{name} {variant}: the scene's own camera in between differs in {_same(second, own, fields)}"
    assert _same(first, own, ("samples",)), f"{name} {variant}: the variant's camera gives the class's own samples"
    assert gs.launch_status() == 0
    gs.close()
    sc.free()
    vsc.free()


def table_lines():
    lines = ["trace / pixel form x variant at %d x %d, depth %d: pixels S = %d from sample %d, rays S = %d; paths, casts and counters equal to the "
             "compiled reference," % (V.W, V.H, V.DEPTH, V.PIXEL_S, V.PIXEL_S0, V.RAY_S),
             "every sample inside trace_expected.value_bar.  Per case: the worst |got - ref| / bar of the ray list, of the pixel list",
             "(measured; the bar is derived in tests/test_gpu_trace.py and does not follow these).", "",
             "  %-24s %s  own  moved in" % ("form", " ".join("%-10s" % v for v in VARIANTS))]
    for kind in ("trace", "pixel"):
        for form in [f for f in V.FORMS if f.startswith("pt_trace_rays" if kind == "trace" else "pt_trace_pixels")]:
            own = {v for (n, v), r in RECORD.items() if r[kind] == form and form in V.CLASSES[n][2:4]}
            moved_in = sorted(f"{n}:{v}" for (n, v), r in RECORD.items() if r[kind] == form and form not in V.CLASSES[n][2:4])
            lines.append("  %-24s %s  %3d  %s" % (form, " ".join("%-10s" % ("ok" if v in own else "-") for v in VARIANTS), len(own),
                                                  ", ".join(moved_in)))
    lines += ["", "  %-14s %-50s %s" % ("class", "forms", " ".join("%-19s" % v for v in VARIANTS))]
    for name in V.CLASS_NAMES:
        cells = []
        for v in VARIANTS:
            r = RECORD.get((name, v))
            cells.append("%-19s" % ("-" if r is None else "%.1e %.1e%s" % (r["rays"], r["pixels"], "*" if (name, v) in V.TRACE_MOVES else "")))
        lines.append("  %-14s %-50s %s" % (name, " / ".join(V.CLASSES[name][2:4]), " ".join(cells)))
    lines.append("  (* the launch took the forms trace_view_scenes.TRACE_MOVES names: %s)" %
                 "; ".join(f"{n} {v} -> {' / '.join(f)}" for (n, v), f in V.TRACE_MOVES.items()))
    return lines


def test_zz_every_kernel_was_compared_under_at_least_eight_variants(gpu):
    """last in this file: the tally of the comparisons above that passed, by the forms the launches took"""
    from rt_amd import abi
    shim = abi.load_shim()
    forms = [shim.rt_hip_trace_kernel_launches(k, None).decode() for k in range(shim.rt_hip_trace_kernel_count())] + \
            [shim.rt_hip_pixel_kernel_launches(k, None).decode() for k in range(shim.rt_hip_pixel_kernel_count())]
    assert sorted(forms) == sorted(V.FORMS) and len(forms) == 10
    lines = table_lines()
    print("\n" + "\n".join(lines))
    print("wall time since the module's first test: %.1f s" % (time.time() - T0[0]))
    short = []
    for form in forms:
        kind = "trace" if form.startswith("pt_trace_rays") else "pixel"
        seen = {v for (n, v), r in RECORD.items() if r[kind] == form}
        if len(seen) < 8 or not seen >= set(VARIANTS) - {"tiny"}:
            short.append((form, sorted(seen)))
    assert not short, f"kernels compared under fewer than 8 variants: {short}"
    missing = [(n, v) for n in V.CLASS_NAMES for v in VARIANTS if (n, v) not in RECORD]
    assert not missing, f"classes not compared under every variant: {missing}"

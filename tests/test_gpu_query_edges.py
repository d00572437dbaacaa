"""Ray queries on the GPU (rt_hip_query_*) where their conservative skipping rules are tightest, BIT FOR BIT against the compiled
reference (tests/query_expected.py) on the ray sets of tests/query_edge_rays.py: every form under the nine cameras and placements of
util.VARIANTS, (u, v) rays and world rays, with three origin_radius hints; origins on a ladder of radii around near_R and around the
sign-test form's near_R sqrt(0.9999), and a fixed set under the hints that move those thresholds across it; sphere silhouettes,
triangle vertices and edges on every form; axis-parallel rays (zeros as 0.0 and -0.0) through vertices and across the widened slab
planes of the hierarchy; origin_radius up to the refusal at near_R = 1e15.  tests/test_query_edges_cpu.py shows what the sets reach.
The closing tests print the table of forms by variant and of rays hit, missed and won by triangles per family
(profiles/r15_query_edges.txt is that print) and assert that every form was compared here."""
import ctypes as C

import numpy as np
import pytest

import query_edge_rays as E
import query_expected as Q
import util

pytestmark = pytest.mark.gpu

COMPARED = set()   # query forms launched by a test of this module that compared their answers
SEEN = {}          # form -> {variant: scene}
FAMILIES = []      # (family, case, form, rays, hit, missed, won by triangles, launches compared)
GRAZE_SCENES = ("rays", "big", "tri", "tri_big", "mem", "lopsided", "soup")


@pytest.fixture
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
    return {f: (a.view(np.uint32) if a.dtype == np.int32 else a) for f, a in res.items()}


def _check(gs, got, exp, what, fields=Q.FIELDS):
    msg = Q.mismatch(got, exp, fields)
    assert not msg, f"{what}: {msg}"
    assert gs.launch_status() == 0
    COMPARED.add(gs.query_kernel_name())


def _record(family, case, gs, exp, launches):
    hit = exp["status"] == 1
    FAMILIES.append((family, case, gs.query_kernel_name(), len(hit), int(hit.sum()), int((exp["status"] == 0).sum()),
                     int((hit & (exp["prim"] != Q.NO_HIT)).sum()), launches))


_CACHE = {}


def _scene(gpu, name):
    """the scene (`name` of Q.SCENES, or name:placement) and its GpuScene: built once, shared, never changed"""
    if name not in _CACHE:
        base, _, variant = name.partition(":")
        sc = Q.SCENES[base][1]()
        if variant:
            own, sc = sc, util.view_variant(sc, variant)
            own.free()
        _CACHE[name] = (sc, gpu.GpuScene(sc))
    return _CACHE[name]


def _farthest(rays):
    return float(np.sqrt((rays[:, :3] ** 2).sum(axis=1)).max())


@pytest.mark.parametrize("name", E.FORM_SCENES)
def test_every_form_under_every_view_and_placement(gpu, ref_mesh, name):
    ref = ref_mesh(5)
    for variant in util.VARIANTS:
        vr = E.variant_rays(name, variant)
        sc, what = vr["scene"], f"{name} {variant}"
        gs = gpu.GpuScene(sc)
        assert gs.query_kernel_name() == E.form_under(name, variant), what   # (E.QUERY_MOVES: the pairs that change form, and why)
        exp = Q.expected(ref, sc, uv=vr["uv"])
        _check(gs, _np(gs.query_uv(vr["uv"])), exp, what + " uv")
        _record("views uv", what, gs, exp, 1)
        exp = Q.expected(ref, sc, rays=vr["rays"])
        far = _farthest(vr["rays"])
        for hint in (None, far, 4.0 * far):
            _check(gs, _np(gs.query_rays(vr["rays"], origin_radius=hint)), exp, f"{what} rays, origin_radius {hint}")
        _record("views rays", what, gs, exp, 3)
        SEEN.setdefault(gs.query_kernel_name(), {})[variant] = name
        assert gs.launch_status() == 0
        gs.close()
        sc.free()


@pytest.mark.parametrize("name", ["rays", "tri", "big", "tri_big", "mem", "lopsided"])
def test_origins_in_the_shell_around_near_R(gpu, ref_mesh, name):
    ref = ref_mesh(5)
    sc, gs = _scene(gpu, name)
    for hint in (0.0, 3.0 * E.reach_of(sc)):
        rays, _ = E.shell_rays(sc, hint)
        exp = Q.expected(ref, sc, rays=rays)
        _check(gs, _np(gs.query_rays(rays, origin_radius=hint)), exp, f"{name} shell around near_R, origin_radius {hint}")
        _record("shell", f"{name} origin_radius {hint:.4g}", gs, exp, 1)
    # a fixed set, every |o| = R0, under the hints that put near_R (and near_R sqrt(0.9999)) just inside, at and just outside R0:
    # each answer is the reference's, so every hint gives the bits of every other
    rays, _ = E.fixed_shell(sc)
    exp = Q.expected(ref, sc, rays=rays)
    hints = E.hint_ladder(sc, rays)
    for hint in hints:
        _check(gs, _np(gs.query_rays(rays, origin_radius=hint)), exp, f"{name} fixed shell, origin_radius {hint!r}")
    _record("hint ladder", name, gs, exp, len(hints))
    assert gs.launch_status() == 0


@pytest.mark.parametrize("name", GRAZE_SCENES)
def test_grazing_rays_on_every_form(gpu, ref_mesh, name):
    sc, gs = _scene(gpu, name)
    rays, _ = E.grazing_rays(sc)
    exp = Q.expected(ref_mesh(5), sc, rays=rays)
    for hint in (None, _farthest(rays)):
        _check(gs, _np(gs.query_rays(rays, origin_radius=hint)), exp, f"{name} grazing, origin_radius {hint}")
    _record("grazing", name, gs, exp, 2)
    assert gs.launch_status() == 0


@pytest.mark.parametrize("case", GRAZE_SCENES + ("tri_big:far", "tri_big:tiny"))
def test_axis_parallel_rays_on_every_form(gpu, ref_mesh, case):
    sc, gs = _scene(gpu, case)
    rays, _, hint = E.axis_set(sc, util.SCALES.get(case.partition(":")[2], 1.0))
    exp = Q.expected(ref_mesh(5), sc, rays=rays)
    for h in (hint, None):   # every origin inside near_R (the slab tests decide), then the default (the farther origins keep all)
        _check(gs, _np(gs.query_rays(rays, origin_radius=h)), exp, f"{case} axis-parallel, origin_radius {h}")
    _record("axis", case, gs, exp, 2)
    assert gs.launch_status() == 0


@pytest.mark.parametrize("name", ["tri", "tri_big"])
def test_origin_radius_up_to_the_limit(gpu, ref_mesh, name):
    sc, gs = _scene(gpu, name)
    rays = Q.ray_set(sc)[:512]
    given = rays.copy()
    exp = Q.expected(ref_mesh(5), sc, rays=rays)
    reach = E.reach_of(sc)
    last = (1e15 * (1.0 - 2e-9) - 1.0) / 1.5 - reach     # the restatement is the shim's to rounding: 1e-9 either side of the limit
    first_refused = (1e15 * (1.0 + 2e-9) - 1.0) / 1.5 - reach
    assert 1e15 * (1.0 - 4e-9) < E.near_R_of(sc, last) < 1e15 * (1.0 - 1e-9)
    assert E.near_R_of(sc, first_refused) >= 1e15 * (1.0 + 1e-9)
    for hint in (reach * 1e3, reach * 1e6, reach * 1e9, reach * 1e12, last):
        _check(gs, _np(gs.query_rays(rays, origin_radius=hint)), exp, f"{name} origin_radius {hint!r}")
    with pytest.raises(gpu.ShimError):
        gs.query_rays(rays, origin_radius=first_refused)
    assert (rays.view(np.uint64) == given.view(np.uint64)).all() and gs.query_kernel_name() == Q.SCENES[name][0]
    _check(gs, _np(gs.query_rays(rays)), exp, f"{name} after the refusal")
    _record("origin_radius up to the limit", name, gs, exp, 6)
    assert gs.launch_status() == 0


def test_zz_every_form_met_the_variants(gpu):
    print("\nquery form x variant (tests/test_gpu_query_edges.py): the scene of query_expected.SCENES compared under it, bit for bit")
    print("  %-24s" % "form" + "".join("%-11s" % v for v in util.VARIANTS) + " variants")
    for form in sorted(SEEN):
        print("  %-24s" % form + "".join("%-11s" % SEEN[form].get(v, "-") for v in util.VARIANTS) + " %d" % len(SEEN[form]))
    print("\n  %-30s %-28s %-22s %6s %6s %6s %9s %9s" % ("family", "case", "form", "rays", "hit", "missed", "triangle", "launches"))
    for row in FAMILIES:
        print("  %-30s %-28s %-22s %6d %6d %6d %9d %9d" % row)
    forms = {Q.SCENES[name][0] for name in E.FORM_SCENES}
    assert set(SEEN) == forms
    for form in forms:
        assert len(SEEN[form]) >= 8, f"{form}: compared under {sorted(SEEN[form])} only"


def test_zz_every_query_form_was_compared_here(gpu):
    from rt_amd import abi
    shim = abi.load_shim()
    for k in range(shim.rt_hip_query_kernel_count()):
        n = C.c_uint64(0)
        name = shim.rt_hip_query_kernel_launches(k, C.byref(n)).decode()
        assert n.value > 0 and name in COMPARED, f"{name}: {n.value} launches, compared: {name in COMPARED}"
    for sc, gs in _CACHE.values():
        gs.close()
        sc.free()
    _CACHE.clear()

"""What the pixel and ray lists of tests/trace_view_scenes.py reach under the view and placement variants (util.VARIANTS), from the
oracles alone.

tests/test_gpu_trace_views.py compares the ten path-tracing query kernels with the compiled reference on these lists, per class and
variant.  A green run of it means something only if the lists make the kernels run what they can get wrong; here the very lists the
device traces (the pixel list at S = 5, sample_first = 3; the ray list at S = 3) are traced by the compiled reference, and the first
scan of every sample is held against conditions fixed beforehand (trace_view_scenes.first_hits: the first scan is a cheap witness,
the paths meet more):

  - every reference sample is finite, and the compiled reference and PtOracle agree on the rays and tests of every sample used
    (expected_pixels / reference_samples with casts_oracle assert it: the casts the device is held to are derivable);
  - summed over its nine variants each class meets: a refractive hit that the roulette lets go on (a path that splits) where it
    has M_REFRACTION, on its M_REFLECTION | M_REFRACTION sphere where it has one; both checker factors where it has M_CHECKERED; a
    triangle where it has a mesh; a miss where its back is open; and where its mesh is checkered a checkered hit whose hit.u /
    hit.v are NOT the winner's own but the last passing triangle's (TriLast);
  - per variant the two lists together hold at least 3 first hits on a material other than M_DEFAULT; the telephoto frame, 6e-5
    across, is asserted to be what it is: its camera rays see at most two objects, and no triangle where a mesh is aimed past.

The TriLast condition was first stated for a checkered SPHERE hit by a ray that passed a triangle.  class_scene's one checkered
sphere is a wall, which lies behind every triangle, so no ray of any list can meet that; the route is the same for a checkered
triangle in front of another triangle of higher index, which is what the lists hold (trace_view_scenes.aimed_rays builds four such
rays per class; the random rays add some).
"""
import numpy as np
import pytest

import refine_expected as R
import trace_expected as T
import trace_view_scenes as V
from util import VARIANTS

M_DEFAULT, M_REFLECTION, M_REFRACTION, M_CHECKERED = 2, 4, 8, 16
_MET = {}


def met(ref_mesh, pt, name):
    """variant -> dict(rays, pixels: first_hits of every sample of the two lists; n_cam: how many leading entries of `rays` are the
    camera rays' samples), computed once per session"""
    if name not in _MET:
        ref, out = ref_mesh(V.DEPTH), {}
        for variant in VARIANTS:
            sc = V.scene_under(name, variant)
            o, q = V.ray_list(sc, name, variant)
            assert 65 <= len(o) <= 73
            rr = T.reference_samples(ref, sc, o, q, V.RAY_S, V.SEED, casts_oracle=pt)
            px = V.pixel_list()
            assert 36 <= len(px) <= 44
            rp = R.expected_pixels(ref, sc, px, V.PIXEL_S, V.PIXEL_S0, V.SEED, casts_oracle=pt)
            assert np.isfinite(rr["samples"]).all() and np.isfinite(rp["samples"]).all(), (name, variant)
            assert np.isfinite(rr["rays"]).all() and (rp["status"] == 2).sum() == 2
            dd = (rr["rays"][:, 3:] ** 2).sum(axis=1)
            assert (np.abs(dd - 1.0) <= 2.0 ** -40).all(), (name, variant)     # unit rays: scanned with the conservative rules
            fr = V.first_hits(ref, pt, sc, np.repeat(rr["rays"], V.RAY_S, axis=0),
                              [(i, s) for i in range(len(o)) for s in range(V.RAY_S)], V.SEED)
            prays, pstreams = V.pixel_sample_rays(ref, pt, sc, px, V.PIXEL_S, V.PIXEL_S0, V.SEED)
            fp = V.first_hits(ref, pt, sc, prays, pstreams, V.SEED)
            out[variant] = dict(rays=fr, pixels=fp, n_cam=V.N_UV * V.RAY_S, ray_paths=rr["paths"], pixel_paths=rp["paths"])
            sc.free()
        _MET[name] = out
    return _MET[name]


def _count(m, cond):
    """how many samples of both lists, over the given variants' records, satisfy cond(first_hits dict) -> bool array"""
    return sum(int(cond(rec[k]).sum()) for rec in m for k in ("rays", "pixels"))


def test_the_class_table_covers_every_form_and_the_moves_are_the_scenes_own():
    from rt_amd import abi
    shim = abi.load_shim()
    trace = [shim.rt_hip_trace_kernel_launches(k, None).decode() for k in range(shim.rt_hip_trace_kernel_count())]
    pixel = [shim.rt_hip_pixel_kernel_launches(k, None).decode() for k in range(shim.rt_hip_pixel_kernel_count())]
    assert len(set(V.CLASS_NAMES)) == len(V.CLASS_NAMES)
    assert {c[2] for c in V.TRACE_VIEW_CLASSES} == set(trace) and {c[3] for c in V.TRACE_VIEW_CLASSES} == set(pixel)
    assert sorted(V.FORMS) == sorted(trace + pixel) and len(V.FORMS) == 10
    assert (V.W, V.H) == (31, 23) and V.DEPTH == 4
    moved = {}
    for name, kw, tf, pf, glass in V.TRACE_VIEW_CLASSES:
        assert pf == tf.replace("pt_trace_rays", "pt_trace_pixels")
        base = V.scene_under(name)
        assert V.picked_forms(base) == (tf, pf), (name, V.picked_forms(base))      # the pick, restated from pt_trace_pick
        assert V.has_refraction(base) == glass, name
        base.free()
        for variant in VARIANTS:
            sc = V.scene_under(name, variant)
            got = V.picked_forms(sc)
            if got != (tf, pf):
                moved[(name, variant)] = got
            sc.free()
    assert moved == V.TRACE_MOVES
    # only `tiny` moves a class, and only a wide one: every form keeps its own class under at least 8 of the 9 variants
    assert all(v == "tiny" and V.CLASSES[n][1].get("wide") for n, v in V.TRACE_MOVES)
    for form in V.FORMS:
        own = [n for n in V.CLASS_NAMES if form in V.CLASSES[n][2:4]]
        assert any(sum(form in V.forms_under(n, v) for v in VARIANTS) >= 8 for n in own), form


def test_the_uv_points_hold_the_corners_the_middle_and_points_outside():
    uv = V.uv_points()
    rows = {tuple(r) for r in uv.tolist()}
    assert {(0.0, 0.0), (1.0, 0.0), (0.0, 1.0), (1.0, 1.0), (0.5, 0.5)} <= rows and len(rows) == V.N_UV
    out = ((uv < 0) | (uv > 1)).any(axis=1)
    assert out.sum() == 8 and (uv[out].min() < 0) and (uv[out].max() > 1)


@pytest.mark.parametrize("name", V.CLASS_NAMES)
def test_each_class_meets_its_materials_over_its_variants(ref_mesh, pt, name):
    kw = V.CLASSES[name][1]
    recs = list(met(ref_mesh, pt, name).values())
    alive = lambda f: f["hit"] & f["alive"]                                                        # noqa: E731
    has = lambda bit: (lambda f: alive(f) & ((f["flags"] & bit) == bit))                           # noqa: E731
    if V.CLASSES[name][4]:
        assert _count(recs, has(M_REFRACTION)) >= 3, f"{name}: no refractive first hit goes on"
        # ... and the split shows in the counters: more trace_path calls than S samples of depth + 2 calls each can make
        assert any((rec["ray_paths"] > V.RAY_S * (V.DEPTH + 2)).any() or (rec["pixel_paths"] > V.PIXEL_S * (V.DEPTH + 2)).any()
                   for rec in recs), name
    else:
        assert all((rec["ray_paths"] <= V.RAY_S * (V.DEPTH + 2)).all() and (rec["pixel_paths"] <= V.PIXEL_S * (V.DEPTH + 2)).all()
                   for rec in recs), name
    if kw.get("glass2"):
        assert _count(recs, has(M_REFLECTION | M_REFRACTION)) >= 3, f"{name}: the M_REFLECTION | M_REFRACTION sphere is not met"
    if kw.get("chk") or kw.get("mesh_chk"):
        assert _count(recs, lambda f: has(M_CHECKERED)(f) & f["on"]) >= 3, f"{name}: no checkered hit with the factor 0.7"
        assert _count(recs, lambda f: has(M_CHECKERED)(f) & ~f["on"]) >= 3, f"{name}: no checkered hit with the factor 0.3"
    if kw.get("chk"):
        assert _count(recs, lambda f: has(M_CHECKERED)(f) & ~f["tri"]) >= 3, f"{name}: the checkered wall is not met"
    if kw.get("tris"):
        assert _count(recs, lambda f: f["tri"]) >= 3, f"{name}: no triangle is a first hit"
    else:
        assert _count(recs, lambda f: f["tri"]) == 0
    if kw.get("mesh_chk"):
        assert _count(recs, lambda f: has(M_CHECKERED)(f) & f["tri"] & f["stale"]) >= 3, f"{name}: no TriLast hit"
    if kw.get("mesh_refr"):
        assert _count(recs, lambda f: has(M_REFRACTION)(f) & f["tri"]) >= 3, f"{name}: no glass triangle is met"
    if kw.get("open_back"):
        assert _count(recs, lambda f: ~f["hit"]) >= 3, f"{name}: no first ray misses"
    else:
        assert _count(recs, lambda f: ~f["hit"]) == 0, f"{name}: a miss in a closed room"


@pytest.mark.parametrize("name", V.CLASS_NAMES)
def test_every_variant_meets_other_materials_and_telephoto_is_what_it_is(ref_mesh, pt, name):
    kw = V.CLASSES[name][1]
    for variant, rec in met(ref_mesh, pt, name).items():
        n = _count([rec], lambda f: f["hit"] & (f["flags"] != M_DEFAULT))
        assert n >= 3, f"{name} {variant}: {n} first hits on a material other than M_DEFAULT"
        # the camera's own rays reach the scene too: some sample of the camera rays or of the pixel list hits
        assert rec["rays"]["hit"][:rec["n_cam"]].any() and rec["pixels"]["hit"].any(), (name, variant)
    tele = met(ref_mesh, pt, name)["telephoto"]
    inside = np.arange(tele["n_cam"]) // V.RAY_S < 5       # the corners and the middle (the points outside [0, 1] see more)
    seen = set(tele["pixels"]["id"].tolist()) | set(tele["rays"]["id"][:tele["n_cam"]][inside].tolist())
    assert len(seen - {-1}) <= 2, f"{name}: a frame 6e-5 across sees objects {sorted(seen)}"
    if kw.get("tris"):      # aimed past the mesh's ball
        assert not tele["pixels"]["tri"].any() and not tele["rays"]["tri"][:tele["n_cam"]][inside].any(), name
    else:                   # aimed at the first packed sphere's silhouette: it or what lies behind it
        assert len(seen - {-1}) >= 1

"""What the first-hit buffers hold under the view and placement variants (util.VARIANTS), from the compiled reference alone.

tests/test_gpu_aov_views.py compares every AOV form with the reference under every variant, whole images, bit for bit.  That
comparison is only worth something if the frames show the AOV kernels what they can get wrong; here each class's nine frames
(util.AOV_FORM_CLASSES at util.AOV_VIEW_SIZE -- the very scenes the device renders) are computed once with
aov_expected.expected_image and held against conditions that were fixed before any frame was looked at:

  - every frame has a pixel that every sample hits, and no two variants of a class give equal buffers;
  - far: some pixel's fp64 distance is no float32 (the rounding in `depth` happens); tiny / huge: depths below 1 / above 1e3;
  - mesh classes: a triangle is the first hit in some pixel under at least 5 of the 9 variants, `inside` among them;
  - _chk classes: a checkered object is hit, with its 0.3x and its 0.7x albedo both, under at least 5 variants;
  - some frame has a pixel that only part of its samples hit.

The room of class_scene is closed: as first measured (40 x 24, 2 samples) no frame of any class held a miss, so the last
condition failed for every class.  The scenes were changed for it, not the condition: two classes (pt_aov_tiles_chk,
pt_aov_tiles_tri_big) lost their back wall (class_scene's open_back), and the size went to 64 x 40 so that the sheared frames of
the 40-triangle classes show more than a handful of triangle pixels.  The frames that contain misses are named by the last test.
"""
import numpy as np
import pytest

from aov_expected import expected_image, mismatch
from conftest import SEED
from util import AOV_FORM_CLASSES, AOV_MOVES, AOV_VIEW_SIZE, VARIANTS, aov_form_under, aov_view_scene

FORM_IDS = [f for f, _ in AOV_FORM_CLASSES]
_FRAMES = {}


def frames(ref_mesh, form):
    """variant -> (expected buffers, extra, n_spheres) of the form's class, computed once per session"""
    if form not in _FRAMES:
        cls = dict(AOV_FORM_CLASSES)[form]
        out = {}
        for variant in VARIANTS:
            sc = aov_view_scene(cls, variant)
            extra = {}
            out[variant] = (expected_image(ref_mesh(5), sc, SEED, sc.samples, extra=extra), extra, sc.n_objects)
            sc.free()
        _FRAMES[form] = out
    return _FRAMES[form]


def test_the_class_list_names_every_form_once_and_the_size_is_not_below_the_floor():
    assert len(set(FORM_IDS)) == len(FORM_IDS) == 10
    assert AOV_VIEW_SIZE["width"] >= 40 and AOV_VIEW_SIZE["height"] >= 24 and AOV_VIEW_SIZE["samples"] >= 2
    assert all(f in FORM_IDS and v in VARIANTS and to in FORM_IDS and to != f for (f, v), to in AOV_MOVES.items())
    # only `tiny` moves a class, and only a wide one; so every form keeps at least 8 of the 9 variants
    for f, cls in AOV_FORM_CLASSES:
        moved = [v for v in VARIANTS if aov_form_under(f, v) != f]
        assert moved in ([], ["tiny"]) and (not moved or cls.get("wide")), (f, moved)


@pytest.mark.parametrize("form", FORM_IDS)
def test_every_frame_is_hit_and_no_two_variants_agree(ref_mesh, form):
    fr = frames(ref_mesh, form)
    S = AOV_VIEW_SIZE["samples"]
    for v, (e, _, _) in fr.items():
        assert (e["hits"] == S).any(), f"{form} {v}: no pixel with every sample hitting"
        full = e["hits"] == S
        assert np.isfinite(e["depth"][e["hits"] > 0]).all() and (e["depth"][e["hits"] == 0] == np.inf).all()
        assert (e["object"][e["hits"] == 0] == 0xFFFFFFFF).all() and (e["object"][e["hits"] > 0] != 0xFFFFFFFF).all()
        n = np.linalg.norm(e["normal"][full].astype(np.float64), axis=1)
        assert n.max() <= 1 + 1e-6 and n.max() > 0.99, f"{form} {v}: mean normals of length up to {n.max()}"
    names = list(fr)
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            assert mismatch(fr[a][0], fr[b][0]), f"{form}: {a} and {b} give equal buffers"


@pytest.mark.parametrize("form", FORM_IDS)
def test_placements_reach_the_depth_s_rounding_and_range(ref_mesh, form):
    fr = frames(ref_mesh, form)
    t = fr["far"][1]["t_min"]
    t = t[np.isfinite(t)]
    inexact = t != t.astype(np.float32).astype(np.float64)
    assert inexact.any(), f"{form} far: every fp64 distance is a float32"
    for v, ok in (("tiny", lambda d: d < 1), ("huge", lambda d: d > 1e3)):
        d = fr[v][0]["depth"]
        d = d[np.isfinite(d)]
        assert d.size and ok(d).all(), f"{form} {v}: depths {d.min()} .. {d.max()}"
    # the scaled frames are the far frame's picture: the same objects in the same pixels (scaling by a power of ten is not
    # exact, so a silhouette sample may change sides -- a handful of pixels at most)
    same = (fr["tiny"][0]["object"] == fr["huge"][0]["object"]).mean()
    assert same > 0.99, f"{form}: tiny and huge disagree on {1 - same:.3f} of the object ids"


@pytest.mark.parametrize("form", [f for f, c in AOV_FORM_CLASSES if c.get("tris")])
def test_mesh_classes_show_triangles_as_first_hits(ref_mesh, form):
    fr = frames(ref_mesh, form)
    seen = [v for v, (e, _, ns) in fr.items() if ((e["hits"] > 0) & (e["object"] >= ns) & (e["object"] != 0xFFFFFFFF)).any()]
    assert "inside" in seen and len(seen) >= 5, f"{form}: a triangle is the first hit only under {seen}"
    assert "telephoto" not in seen, f"{form}: the telephoto frame is aimed past the mesh's ball"


@pytest.mark.parametrize("form", [f for f in FORM_IDS if f.endswith("_chk")])
def test_chk_classes_show_both_checker_albedos(ref_mesh, form):
    fr = frames(ref_mesh, form)
    both = [v for v, (_, x, _) in fr.items() if (x["checker"][:, 0] > 0).any() and (x["checker"][:, 1] > 0).any()]
    assert len(both) >= 5, f"{form}: a checkered first hit with both the 0.3x and the 0.7x albedo only under {both}"


def test_some_frame_has_a_silhouette_inside_a_pixel_and_the_frames_with_misses_are_named(ref_mesh):
    S = AOV_VIEW_SIZE["samples"]
    partial, misses = [], []
    for form, cls in AOV_FORM_CLASSES:
        for v, (e, _, _) in frames(ref_mesh, form).items():
            p, m = int(((e["hits"] > 0) & (e["hits"] < S)).sum()), int((e["hits"] == 0).sum())
            if p:
                partial.append((form, v, p))
            if m:
                misses.append((form, v, m))
                assert cls.get("open_back"), f"{form} {v}: {m} pixels miss in a closed room"
    print("\nframes with pixels that part of the samples hit:", *(f"\n  {f:26s} {v:10s} {n:5d}" for f, v, n in partial))
    print("frames with pixels that nothing hits:", *(f"\n  {f:26s} {v:10s} {n:5d}" for f, v, n in misses))
    assert partial, "no frame has a pixel with 0 < hits < samples"
    assert misses, "no frame has a miss"
    # each open class shows misses under its own placement variants (the class camera faces the missing wall)
    for form, cls in AOV_FORM_CLASSES:
        if cls.get("open_back"):
            assert {v for f, v, _ in misses if f == form} >= {"far", "tiny", "huge"}, form
            assert any(f == form for f, _, _ in partial), form

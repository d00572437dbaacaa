"""What the ray sets of tests/query_edge_rays.py reach, on the compiled reference's answers alone (no GPU): each condition here is
what keeps a comparison of tests/test_gpu_query_edges.py from passing vacuously.  The cost of query_expected.expected() for every set
is printed (-s): it stays at the scale of the existing query tests, a few seconds a test."""
import time

import numpy as np
import pytest

import query_edge_rays as E
import query_expected as Q
import util

GRAZE_SCENES = ("rays", "big", "tri", "tri_big", "mem", "lopsided", "soup")
SHELL_SCENES = ("rays", "tri", "big", "tri_big", "mem", "lopsided")
AXIS_CASES = GRAZE_SCENES + ("tri_big:far", "tri_big:tiny")


def _counts(exp):
    hit = exp["status"] == 1
    tri = hit & (exp["prim"] != Q.NO_HIT)
    return hit, tri


def _timed_expected(ref, sc, what, **kw):
    t0 = time.time()
    exp = Q.expected(ref, sc, **kw)
    hit, tri = _counts(exp)
    print(f"{what}: {len(hit)} rays, {hit.sum()} hit, {(exp['status'] == 0).sum()} miss, {tri.sum()} won by triangles, expected() {time.time() - t0:.2f} s")
    return exp


@pytest.mark.parametrize("name", E.FORM_SCENES)
def test_every_variant_set_is_valid_hits_and_meets_the_same_geometry_when_scaled(ref_mesh, name):
    ref = ref_mesh(5)
    base = None
    for variant in (None,) + util.VARIANTS:
        vr = E.variant_rays(name, variant)
        sc, what = vr["scene"], f"{name} {variant or 'own'}"
        eu = _timed_expected(ref, sc, what + " uv", uv=vr["uv"])
        er = _timed_expected(ref, sc, what + " rays", rays=vr["rays"])
        both = {f: np.concatenate([eu[f], er[f]]) for f in Q.FIELDS}
        assert (both["status"] != 2).all(), what
        hit, tri = _counts(both)
        assert hit.sum() >= 0.25 * len(hit), what
        if sc.n_meshes:
            assert tri.sum() >= 8 and (hit & ~tri).sum() >= 8, f"{what}: {tri.sum()} triangle winners, {(hit & ~tri).sum()} sphere winners"
        if name in E.OPEN_BACK:
            if (name, variant) in E.SEALED:
                assert len(vr["uv"]) == len(E.uv_set()) and len(E.opening_uv(sc, vr["scale"])) == 0, what   # none of 9600 escapes
            else:
                assert (eu["status"] == 0).sum() >= 0.1 * len(vr["uv"]), f"{what}: {(eu['status'] == 0).sum()} of {len(vr['uv'])} uv rays miss"
        if variant == "far":
            assert (np.sqrt((both["ray"][:, :3] ** 2).sum(axis=1)) > 2.0 ** 24).all(), what
        if variant is None:
            base = both
        if variant in util.SCALES:   # the same geometry is met (a statement about the sets, no bar for the GPU)
            s = vr["scale"]
            assert (both["status"] == base["status"]).all() and (both["object"] == base["object"]).all(), what
            assert (both["prim"] == base["prim"]).all(), what
            assert (np.abs(both["t"][hit] - s * base["t"][hit]) <= 1e-9 * s * base["t"][hit]).all(), what
        sc.free()


@pytest.mark.parametrize("name", SHELL_SCENES)
def test_shell_sets_bracket_near_R_and_hit(ref_mesh, name):
    ref = ref_mesh(5)
    sc = Q.SCENES[name][1]()
    reach = E.reach_of(sc)
    for hint in (0.0, 3.0 * reach):
        R = E.near_R_of(sc, hint)
        assert R == 1.5 * (hint + reach) + 1.0
        radii = E.ladder(R)
        assert len(radii) == 26 and radii.max() > R * (1.0 + 1e-4) and radii.min() < R * E.SIGN_TEST_FACTOR * (1.0 - 1e-4) < R * (1.0 - 1e-4)
        for c in (R, R * E.SIGN_TEST_FACTOR):   # the finest rungs: 2^-50 to either side of the value (to the rounding of c (1 + x))
            near = np.sort(radii[np.abs(radii / c - 1.0) < 2.0 ** -45])
            assert len(near) == 3 and near[1] == c and (np.abs(np.diff(near) / c / 2.0 ** -50 - 1.0) < 0.3).all(), near
        rays, k = E.shell_rays(sc, hint)
        assert len(rays) == 512 and np.bincount(k, minlength=26).min() >= 16
        r = np.sqrt((rays[:, :3] ** 2).sum(axis=1))
        assert (np.abs(r / radii[k] - 1.0) < 1e-15).all()
        exp = _timed_expected(ref, sc, f"{name} shell, origin_radius {hint:.4g}", rays=rays)
        hit, tri = _counts(exp)
        assert (exp["status"] != 2).all() and hit.sum() >= 256
        assert not sc.n_meshes or tri.sum() >= 8
    rays, R0 = E.fixed_shell(sc)
    assert (np.abs(np.sqrt((rays[:, :3] ** 2).sum(axis=1)) / R0 - 1.0) < 1e-15).all()
    hints = E.hint_ladder(sc, rays)
    at = np.array([E.near_R_of(sc, h) for h in hints]) / R0
    assert len(hints) == 26 and min(hints) >= 0.0 and at.min() < 1.0 - 2.0 ** -11 and at.max() > 1.0 + 2.0 ** -11
    assert (np.abs(at[:13] - 1.0) < 2.0 ** -49).sum() == 3 and (np.abs(at[13:] * E.SIGN_TEST_FACTOR - 1.0) < 2.0 ** -49).sum() == 3
    exp = _timed_expected(ref, sc, f"{name} fixed shell", rays=rays)
    assert _counts(exp)[0].sum() >= 256
    sc.free()


def _triangle15(sc, t):
    v = np.concatenate([m["vertices"] for m in util.scene_parts(sc)[1]])[3 * t:3 * t + 3, :3]
    v15 = np.zeros(15)
    v15[0:3], v15[5:8], v15[10:13] = v
    v15[8], v15[14] = 1.0, 1.0
    return v15


@pytest.mark.parametrize("name", GRAZE_SCENES)
def test_grazing_sets_are_answered_both_ways(ref_mesh, name):
    ref = ref_mesh(5)
    sc = Q.SCENES[name][1]()
    rays, info = E.grazing_rays(sc)
    exp = _timed_expected(ref, sc, f"{name} grazing", rays=rays)
    assert (exp["status"] != 2).all()
    hit, tri = _counts(exp)
    close = (info["kind"] == 0) & (np.abs(info["delta"]) <= 2.0 ** -30)
    own = hit & ~tri & (exp["object"] == info["target"])
    print(f"  silhouettes within 2^-30: {close.sum()}, their sphere wins {(close & own).sum()}, it does not {(close & ~own).sum()}")
    assert close.sum() >= 50 and (close & own).sum() >= 0.1 * close.sum() and (close & ~own).sum() >= 0.1 * close.sum()
    if not sc.n_meshes:
        assert (info["kind"] == 0).all()
        sc.free()
        return
    exact = (info["kind"] == 1) | (info["kind"] == 2)
    b = exp["bary"]
    on_edge = tri & ((b[:, 0] == 0.0) | (b[:, 1] == 0.0) | (np.abs(b[:, 0] + b[:, 1] - 1.0) <= 2.0 ** -40))
    print(f"  exact vertex and edge rays: {exact.sum()}, won by a triangle {(exact & tri).sum()}, on its edge {(exact & on_edge).sum()}")
    assert (exact & on_edge).sum() >= 8
    moved = info["kind"] == 3     # across the edge by +-2^-k: the aimed-at triangle wins on one side more often than on the other
    mine = tri & (exp["prim"] == info["target"])
    assert (moved & mine & (info["delta"] < 0)).sum() > (moved & mine & (info["delta"] > 0)).sum()
    # neighbours with the same t: the lower index wins
    tri_v = np.concatenate([m["vertices"][:, :3] for m in util.scene_parts(sc)[1]]).reshape(-1, 3, 3)
    partner = {}
    for i, j in E.neighbour_pairs(tri_v):
        partner.setdefault(i, []).append(j)
    ties = 0
    for k in np.nonzero(exact & tri)[0]:
        for j in partner.get(int(exp["prim"][k]), []):
            ok, out = ref.intersect_triangle(rays[k], _triangle15(sc, j))
            ties += bool(ok and out[0] == exp["t"][k])
    print(f"  neighbouring triangles with the winner's t (the lower index won): {ties}")
    if name in ("lopsided", "soup"):   # the scenes with exact duplicates (E.neighbour_pairs: the sheets of class_scene share no edge)
        assert ties >= 1, name
    else:
        assert not partner, name
    sc.free()


@pytest.mark.parametrize("case", AXIS_CASES)
def test_axis_sets_have_exact_zeros_and_ladders_that_hit_and_miss(ref_mesh, case):
    ref = ref_mesh(5)
    name, _, variant = case.partition(":")
    sc = Q.SCENES[name][1]()
    if variant:
        base, sc = sc, util.view_variant(sc, variant)
        base.free()
    rays, info, hint = E.axis_set(sc, util.SCALES.get(variant, 1.0))
    d = rays[:, 3:]
    assert (np.abs((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2] - 1.0) <= 2.0 ** -40).all()
    zero = (d == 0.0).any(axis=1)
    minus = ((d == 0.0) & np.signbit(d)).any(axis=1)
    assert zero.sum() >= 64 and minus.sum() >= 16 and (zero & ~minus).sum() >= 16
    exp = _timed_expected(ref, sc, f"{case} axis", rays=rays)
    assert (exp["status"] != 2).all()
    hit, tri = _counts(exp)
    if not sc.n_meshes:
        assert (info["kind"] == 3).all() and hit.sum() >= 0.25 * len(rays)
        sc.free()
        return
    if name in E.HIERARCHY_SCENES:
        assert tri.sum() >= 0.25 * len(rays), f"{case}: {tri.sum()} of {len(rays)} rays are won by a triangle"
    lad = info["kind"] == 2
    assert (lad & tri).sum() >= 1 and (lad & ~tri).sum() >= 1
    for f in range(6):
        m = lad & (info["face"] == f)
        steps = info["step"][m]
        # the steps are consecutive fp32 values of the coordinate across the face, and cover twice the widening (or 512 steps)
        x = np.unique(rays[m][:, f // 2])
        assert (x == x.astype(np.float32)).all() and (np.sign(x) == np.sign(x[0])).all(), (case, f)
        assert (np.diff(np.sort(np.abs(x)).astype(np.float32).view(np.int32).astype(np.int64)) == 1).all(), (case, f)
        edge = rays[m][:, f // 2][steps == 0][0]
        assert steps.max() == E.AXIS_STEPS_MAX or np.abs(x - edge).max() >= 8.0 * E.E24 * (E.near_R_of(sc, hint) + abs(edge)), (case, f)
        inner = m & np.isfinite(info["t_point"])        # passes through a point of the extreme triangle: that or something nearer is hit
        assert inner.any() and (hit[inner] & (exp["t"][inner] <= info["t_point"][inner] * (1.0 + 1e-9))).all(), (case, f)
        assert not tri[m & (info["step"] == steps.max())].any(), (case, f)   # the outermost step passes the mesh
    sc.free()

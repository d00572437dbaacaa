"""The restatements of rt_hip_prev_points and rt_hip_reproject_points (tests/reproject_points_expected.py) without a GPU: the
vectorised and the scalar form of each agree bit for bit; without previous points, and with step 3's own point as the previous
point, the new contract is rt_hip_reproject's; the planted previous points reach what they are planted for; the edge list of
prev_points reaches every branch; and with unmoved positions the blend reproduces a real query's hit point."""
import numpy as np
import pytest

import reproject_expected as RE
import reproject_points_expected as PE


@pytest.mark.parametrize("size", RE.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_reproject_points_restatements(size):
    w, h = size
    for kind, k in RE.CASES:
        seed = RE.case_seed(w, h, kind)
        rgb, aov, cam, hist, pts, _ = PE.planted_points(w, h, kind, seed)
        p = RE.params(k)
        what = f"{w}x{h} {kind} {p}"
        # vectorised == scalar, bit for bit
        vec = PE.reproject(rgb, aov, cam, hist, prev_points=pts, **p)
        msg = RE.mismatch(PE.scalar_reproject(rgb, aov, cam, hist, prev_points=pts, **p), vec)
        assert not msg, f"{what}: {msg}"
        # no previous points: rt_hip_reproject itself
        old_info = {}
        old = RE.reproject(rgb, aov, cam, hist, info=old_info, **p)
        assert not RE.mismatch(PE.reproject(rgb, aov, cam, hist, prev_points=None, **p), old), what
        # step 3's own P as the previous point: rt_hip_reproject on every pixel that reaches step 3 (where P is not finite the old
        # contract goes on to step 4, which then fails every comparison: the same outputs, by another exit)
        own = PE.reproject(rgb, aov, cam, hist, prev_points=PE.step3_points(aov, cam, w, h), **p)
        at = old_info["candidate"]
        for f in ("rgb", "len", "motion"):
            assert RE.same_floats(own[f][at], old[f][at]) if f == "rgb" else RE.same_bits(own[f][at], old[f][at]), f"{what}: {f}"
        assert not RE.mismatch(PE.reproject(rgb, aov, cam, None, prev_points=pts, **p), RE.reproject(rgb, aov, cam, None, **p)), what


def test_planted_points_reach_what_they_are_for():
    """per reason, over every size and camera kind: how many pixels that passed steps 1 and 2 ended where the planted point sends them"""
    count = {r: 0 for r in ("nonfinite", "at_camera", "behind", "out_of_frame", "plus_1e300", "minus_1e300", "denormal", "neg_zero",
                            "sub_pixel_blended", "pixels_away_blended")}
    for w, h in RE.SIZES:
        for kind in ("small", "large"):
            rgb, aov, cam, hist, pts, planted = PE.planted_points(w, h, kind, RE.case_seed(w, h, kind))
            info = {}
            res = PE.reproject(rgb, aov, cam, hist, prev_points=pts, info=info, **RE.DEFAULTS)
            flat = {f: m.reshape(-1) for f, m in info.items()}
            reached = flat["candidate"] | flat["nonfinite_point"]            # passed steps 1 and 2
            pick = lambda cat, m: int((m[planted[cat]] & reached[planted[cat]]).sum())
            count["nonfinite"] += pick("nan", flat["nonfinite_point"]) + pick("inf", flat["nonfinite_point"])
            count["at_camera"] += pick("at_camera", flat["det_zero"] & ~flat["ok"])
            count["behind"] += pick("behind", flat["behind"])
            count["out_of_frame"] += pick("out_of_frame", flat["out_of_frame"])
            for cat in ("plus_1e300", "minus_1e300", "denormal", "neg_zero"):
                count[cat] += pick(cat, flat["candidate"])
            count["sub_pixel_blended"] += pick("sub_pixel", flat["blended"])
            count["pixels_away_blended"] += pick("pixels_away", flat["blended"])
            # a pixel that ends at step 3' keeps its colour, length 1, no motion
            end = info["nonfinite_point"]
            assert RE.same_floats(res["rgb"][end], rgb[end]) and (res["len"][end] == 1).all() and np.isnan(res["motion"][end]).all()
            # the ordinary points move by what they were planted with
            sub = planted["sub_pixel"][flat["ok"][planted["sub_pixel"]]]
            assert (np.abs(res["motion"].reshape(-1, 2)[sub]) < 0.5).all()
    print("\nplanted previous points, pixels per reason:", count)
    assert all(v > 0 for v in count.values()), count


@pytest.mark.parametrize("n_tri", [12, 1, 0])
def test_prev_points_restatements_and_branches(n_tri):
    rng = np.random.default_rng(5 + n_tri)
    tris = PE.edge_positions(rng.normal(size=(n_tri, 3, 3)) * 2.0, seed=n_tri) if n_tri else None
    for n in (0, 1, 63, 64, 65, 257, 2000):
        status, prim, bary, point = PE.edge_hits(n, n_tri, seed=1000 * n_tri + n)
        vec = PE.prev_points(status, prim, bary, point, tris)
        assert PE.same_bits64(vec, PE.scalar_prev_points(status, prim, bary, point, tris)), (n_tri, n)
        hit = status == 1
        assert (vec.view(np.uint64)[~hit] == PE.QNAN64_BITS).all()
        sphere = hit & (prim == PE.NO_PRIM)
        assert (vec.view(np.uint64)[sphere] == point.view(np.uint64)[sphere]).all()          # NaN payloads survive
        if n == 2000:
            counts = PE.branch_counts(status, prim, n_tri)
            assert all(v > 0 for f, v in counts.items() if not (f == "triangle" and n_tri == 0)), counts
            for u in PE.BARY_VALUES:
                same = (bary[:, 0].view(np.uint64) == np.float64(u).view(np.uint64)) & hit & (prim < n_tri)
                assert n_tri == 0 or same.any(), u
    # overflow to inf is a result
    one = PE.prev_points([1], [0], [[1e300, 0.5]], [[0, 0, 0]], [[[1.0, 2.0, 3.0], [1e300, -1e300, 1e10], [0.0, 0.0, 0.0]]])
    assert np.isinf(one[0, 0]) and np.isinf(one[0, 1]) and np.isnan(one).sum() == 0


def test_unmoved_positions_reproduce_the_hit_point(ref_mesh):
    """A real query (the compiled reference's scan, tests/query_expected.py) through the pixel centres of the deforming scene's first
    pose; previous positions = current positions.  The query's point is o + d*t, the blend a*w0 + b*u + c*v: two roundings of one
    point X of the triangle's plane.
      o + d*t: one product and one sum, 2 eps max(|o|, t) per component (|d| <= 1), and t itself carries Moeller-Trumbore's error;
      the blend: three products and three sums on values bounded by the largest corner magnitude Mc, 6 eps Mc, and u, v carry theirs.
    t, u and v are each a quotient of two dot products of differences of the inputs: about 8 roundings, relative to the largest
    term of the sums, which exceeds the result by the conditioning 1 / c of the intersection, c = |d . n| (unit normal n): a ray
    that grazes the triangle cancels.  So with S = max(Mc, |o|, t): |point - blend| <= (2 + 6 + 3 * 8 / c) eps S <= 32 eps S / c for
    c <= 1.  The rays kept are those with c >= 1/4 (the others are counted, not bounded)."""
    import query_expected as QE
    w, h = 24, 14
    tris = PE.wobble_pose(0)
    sc = PE.mesh_scene(tris, w, h, 1)
    exp = QE.expected(ref_mesh(sc.max_depth), sc, uv=PE.pixel_centre_uv(w, h))
    on_mesh = (exp["status"] == 1) & (exp["prim"] != PE.NO_PRIM)
    assert on_mesh.sum() > 20
    got = PE.prev_points(exp["status"], exp["prim"], exp["bary"], exp["point"], tris)
    t = tris[exp["prim"][on_mesh]]
    n = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    c = np.abs((exp["ray"][on_mesh, 3:] * n).sum(axis=1))
    S = np.maximum(np.maximum(np.abs(t).max(axis=(1, 2)), np.abs(exp["ray"][on_mesh, :3]).max(axis=1)), exp["t"][on_mesh])
    err = np.abs(got[on_mesh] - exp["point"][on_mesh]).max(axis=1)
    keep = c >= 0.25
    bound = 32 * 2.0 ** -53 * S / c
    print(f"\nunmoved positions: {int(keep.sum())} of {int(on_mesh.sum())} hits bounded, worst error / bound {float((err[keep] / bound[keep]).max()):.3f}")
    assert keep.sum() > 10 and (err[keep] <= bound[keep]).all()
    sc.free()

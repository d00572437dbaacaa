"""Moving spheres without a device: scene_spheres.h (raytracer.c_amd/csrc), the one text of what a scene derives from its spheres,
run as a stand-alone program under AddressSanitizer and UBSan (tests/sphere_update_harness.cpp) and compared bit for bit with the
numpy restatement (tests/sphere_update_expected.py) where a rule has an edge; the numpy restatement of rt_hip_prev_points_moved's
sphere clause against a scalar one; and the C interface of the feature before any device is touched."""
import ctypes as C

import numpy as np
import pytest

import prev_points_moved_expected as P
import sphere_update_expected as E

UP = np.nextafter


def room():
    """config 4's room: 38 spheres, six of them walls"""
    from rt_amd import scene as S
    sc = S.build_scene(4, 48, 32, 1)
    s = E.spheres_of(sc)
    sc.free()
    assert len(s) == 38
    return s


def walls(k, then=3):
    """k leading wall-sized spheres, then `then` small ones"""
    rng = np.random.default_rng(40 + k)
    w = np.array([[0.0, -(10.0 ** (3 + i % 3)) - 10.0 - i, float(i), 10.0 ** (3 + i % 3)] for i in range(k)]).reshape(-1, 4)
    small = np.concatenate([rng.uniform(-8, 8, (then, 3)), rng.uniform(0.5, 2, (then, 1))], axis=1)
    return np.concatenate([w, small])


def cases():
    r = room()
    out = {"room": r, "empty": np.zeros((0, 4)), "one": np.array([[1.0, 2.0, 3.0, 0.5]])}
    for name, rad in (("r999.9999", 999.9999), ("r1000", 1000.0), ("r1000.0001", 1000.0001), ("r_below_1000", UP(1000.0, 0.0))):
        out[name] = np.array([[3.0, -4.0, 12.0, rad], [0.0, 1.0, 0.0, 2.0]])        # reach: ordinary size is |r| < 1000
    for name, v in (("1e17", 1e17), ("above_1e17", UP(1e17, np.inf))):
        out["radius_" + name] = np.array([[0.0, 0.0, 5.0, 1.0], [1.0, 0.0, 0.0, v]])
        # |c| is rounded UP by (1 + 1e-12): a centre AT 1e17 is already wide; the last one that is not lies below it
        out["centre_" + name] = np.array([[v, 0.0, 0.0, 1.0]])
        out["leading_radius_" + name] = np.array([[0.0, 0.0, 5.0, v], [0.0, 9.0, 0.0, 2000.0]])   # a wall must be <= 1e17
    out["centre_below_1e17"] = np.array([[1e17 / (1.0 + 2e-12), 0.0, 0.0, 1.0]])
    out["negative_radius"] = np.array([[1.0, 2.0, 3.0, -2.5], [0.0, -5000.0, 0.0, -4000.0], [0.0, 5000.0, 0.0, 4000.0]])
    out["minus_zero_centres"] = np.array([[-0.0, 0.0, -0.0, 1.0], [-0.0, -0.0, -0.0, 3.0]])
    out["nan_and_inf_centres"] = np.array([[np.nan, 0.0, 0.0, 1.0], [np.inf, 0.0, 0.0, 1.0], [1.0, 1.0, 1.0, 1.0]])
    out["bad_radii"] = np.array([[0.0, 0.0, 0.0, 1e-101], [0.0, 0.0, 0.0, 1e101], [0.0, 0.0, 0.0, np.nan], [0.0, 0.0, 0.0, 0.0]])
    out["edge_radii"] = np.array([[0.0, 0.0, 0.0, 1e-100], [0.0, 0.0, 0.0, -1e100]])
    for k in (0, 1, 7, 8, 9):
        out[f"walls{k}"] = walls(k)
    out["walls_only_2"] = walls(2, then=0)
    out["wall_after_small"] = np.concatenate([walls(0, then=1), walls(4)])
    for name, move in E.MOVES.items():
        out["room_" + name] = move(r)
    out["room_far"] = E.far_centre(r)
    return out


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    """the sanitized program, run once over every case"""
    c = cases()
    prog = E.compile_harness(tmp_path_factory.mktemp("spheres"))
    return c, dict(zip(c, E.run_harness(prog, list(c.values()))))


@pytest.mark.parametrize("name", list(cases()))
def test_header_equals_the_numpy_restatement(results, name):
    c, got = results
    want = E.expected(c[name])
    assert not E.mismatch(got[name], want), f"{name}: {E.mismatch(got[name], want)}"


def test_the_edges_fall_where_the_rules_say(results):
    c, got = results
    g = lambda k: got[k]
    assert g("room")["n_big"] in (6, 8) and g("room")["reach_spheres"] > 0 and not g("room")["wide_range"]
    # ordinary size is |r| < 1000: at 1000 the sphere no longer counts, and it is a wall (a lone leading wall: no whole pair)
    assert g("r999.9999")["reach_spheres"] == 13.0 * (1.0 + 1e-12) + 999.9999 and g("r_below_1000")["reach_spheres"] > 1012.9
    assert g("r1000")["reach_spheres"] == 1.0 * (1.0 + 1e-12) + 2.0 == g("r1000.0001")["reach_spheres"]
    assert [g(k)["n_big"] for k in ("r999.9999", "r1000", "r1000.0001")] == [0, 0, 0]
    # wide: beyond 1e17, not at it -- but |c| carries its rounding up
    assert not g("radius_1e17")["wide_range"] and g("radius_above_1e17")["wide_range"]
    assert g("centre_1e17")["wide_range"] and g("centre_above_1e17")["wide_range"] and not g("centre_below_1e17")["wide_range"]
    assert g("leading_radius_1e17")["n_big"] == 2 and g("leading_radius_above_1e17")["n_big"] == 0
    # a negative radius: r * r, |r| in the reach and among the walls
    n = g("negative_radius")
    assert n["entry"][0, 3] == 6.25 and n["reach_spheres"] == np.sqrt(14.0) * (1.0 + 1e-12) + 2.5 and n["n_big"] == 0
    z = g("minus_zero_centres")
    assert np.signbit(z["entry"][0, 0]) and not np.signbit(z["entry"][0, 1]) and np.signbit(z["geom4"][1, 2])
    assert z["max_center"] == 0.0 and not np.signbit(z["max_center"]) and z["reach_spheres"] == 3.0
    q = g("nan_and_inf_centres")
    assert q["wide_range"] and q["max_center"] == np.inf and q["reach_spheres"] == np.inf
    assert not g("bad_radii")["radii_ok"] and g("edge_radii")["radii_ok"] and g("room")["radii_ok"]
    # whole pairs of LEADING walls, at most 8; nothing beyond n_big
    assert [g(f"walls{k}")["n_big"] for k in (0, 1, 7, 8, 9)] == [0, 0, 6, 8, 8]
    assert g("walls_only_2")["n_big"] == 2 and g("wall_after_small")["n_big"] == 0
    for k in (1, 7):
        assert (g(f"walls{k}")["big_r"][g(f"walls{k}")["n_big"]:] == 0).all() and (g(f"walls{k}")["big_c"][g(f"walls{k}")["n_big"]:] == 0).all()
    assert g("walls7")["big_r"][5] == 1e5 and g("walls7")["big_c"][0] == 1010.0 * (1.0 + 1e-12)
    # the moves of the GPU test do what it says of them
    r = g("room")
    assert g("room_identity")["reach_spheres"] == r["reach_spheres"]
    assert g("room_translate")["reach_spheres"] > r["reach_spheres"] + 10 and g("room_translate")["n_big"] == r["n_big"]
    assert g("room_wall_shrunk")["n_big"] == 2 and g("room_wall_shrunk")["reach_spheres"] > 1000 > r["reach_spheres"]
    assert g("room_far")["wide_range"] and not g("room_jitter")["wide_range"]
    assert not E.same_bits(g("room_jitter")["entry"], r["entry"]) and E.same_bits(g("room_jitter")["entry"][:6], r["entry"][:6])


def test_prev_points_moved_restatement_against_the_scalar_one():
    rng = np.random.default_rng(3)
    hits, prev, cur = P.planted(6, 5)
    n = 200
    more = dict(status=rng.choice([0, 1, 1, 1, 2], n).astype(np.uint32), prim=rng.choice([P.NO_PRIM, P.NO_PRIM, 0, 4, 5, 9], n).astype(np.uint32),
                object=rng.choice([0, 1, 2, 3, 5, 6, 77], n).astype(np.uint32), bary=rng.uniform(0, 0.5, (n, 2)), point=rng.uniform(-9, 9, (n, 3)))
    both = {f: np.concatenate([hits[f], more[f]]) for f in hits}
    pos = rng.uniform(-4, 4, (5, 3, 3))
    for positions, sp, sc in ((pos, prev, cur), (None, prev, cur), (pos, None, None), (pos, prev[:0], cur[:0])):
        a, b = P.prev_points_moved(both, positions, sp, sc), P.prev_points_moved_scalar(both, positions, sp, sc)
        assert P.same(a, b)
        assert np.isnan(a).any() and np.isfinite(a).any()
    out = P.prev_points_moved(hits, pos, prev, cur)
    bits = out.view(np.uint64)
    assert (bits[[0, 1, 2, 3, 6, 9]] == P.QNAN).all(), "status 0 and 2, object == n_spheres, object 0xFFFFFFFF, a prim out of range"
    assert np.array_equal(out[4], prev[2, :3] + (hits["point"][4] - cur[2, :3]) * 1.0), "r = r': a pure translation"
    assert np.isinf(out[5]).all(), "the radius ratio overflowed"
    still = P.prev_points_moved(hits, pos, None, None)
    assert np.array_equal(still.view(np.uint64)[[2, 3, 4, 5, 8]], hits["point"].view(np.uint64)[[2, 3, 4, 5, 8]]), "no spheres given: the point's bits"
    # the clause itself: a point on the current sphere lands on the previous one, at the same place of its surface
    c, r, c2, r2 = np.array([1.0, 2.0, 3.0]), 2.0, np.array([-4.0, 0.5, 9.0]), 3.0
    d = np.array([0.6, 0.0, 0.8])
    one = dict(status=np.array([1], np.uint32), prim=np.array([P.NO_PRIM], np.uint32), object=np.array([0], np.uint32), bary=np.zeros((1, 2)),
               point=(c + r * d)[None])
    got = P.prev_points_moved(one, None, np.array([[*c2, r2]]), np.array([[*c, r]]))[0]
    assert np.allclose(got, c2 + r2 * d, rtol=0, atol=1e-14)


def test_interface():
    """the symbols in both builds of the shim, abi.py against the header, and the argument errors that need no device"""
    import os
    import re
    from rt_amd import abi
    shim = abi.load_shim()
    names = ("rt_hip_scene_update_spheres", "rt_hip_scene_update_spheres_host", "rt_hip_scene_read_spheres", "rt_hip_scene_sphere_bounds",
             "rt_hip_prev_points_moved", "rt_hip_prev_points_moved_host")
    diag = C.CDLL(os.path.join(os.path.dirname(abi.SHIM_PATH), "librt_hip_diag.so"))
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(E.ROOT, "include", "rt_hip.h")).read(), flags=re.S)
    for name in names:
        assert hasattr(shim, name) and hasattr(diag, name), name
        assert name in abi.SHIM_SYMBOLS and re.search(r"\b%s\s*\(" % name, header), name
    buf = (C.c_double * 8)()
    assert shim.rt_hip_scene_update_spheres(None, buf, 2) == abi.EINVAL
    assert shim.rt_hip_scene_update_spheres_host(None, buf, 2) == abi.EINVAL and b"required" in shim.rt_hip_last_error()
    assert shim.rt_hip_scene_read_spheres(None, None, None) == abi.EINVAL
    assert shim.rt_hip_scene_sphere_bounds(None, None, None, None, None, None, None) == abi.EINVAL
    # rt_hip_prev_points' error order: the arguments first (RT_HIP_EINVAL), then the device (RT_HIP_ENODEV)
    n = 4
    st, pr, ob = (C.c_uint32 * n)(), (C.c_uint32 * n)(), (C.c_uint32 * n)()
    ba, po, out = (C.c_double * (2 * n))(), (C.c_double * (3 * n))(), (C.c_double * (3 * n))()
    sp = (C.c_double * 8)()
    h = abi.RtHipHits()
    h.status, h.prim, h.bary, h.point = C.addressof(st), C.addressof(pr), C.addressof(ba), C.addressof(po)
    host_form = lambda *a: shim.rt_hip_prev_points_moved_host(C.byref(h), n, None, 0, *a)
    assert host_form(sp, sp, 2, 0, out) == abi.EINVAL and b"object" in shim.rt_hip_last_error()
    h.object = C.addressof(ob)
    assert host_form(None, sp, 2, 0, out) == abi.EINVAL and host_form(sp, None, 2, 0, out) == abi.EINVAL
    assert host_form(sp, sp, 2, 0, None) == abi.EINVAL
    assert host_form(sp, sp, 2, 0, sp) == abi.EINVAL and b"overlaps" in shim.rt_hip_last_error()
    assert shim.rt_hip_prev_points_moved(C.byref(h), 1 << 32, None, 0, None, None, 0, out, None) == abi.EINVAL
    assert shim.rt_hip_prev_points_moved_host(C.byref(h), 0, None, 0, None, None, 0, 99, out) in (abi.ENODEV, abi.EINVAL)
    if shim.rt_hip_device_count() == 0:
        assert host_form(sp, sp, 2, 0, out) == abi.ENODEV
        assert host_form(None, None, 0, 0, out) == abi.ENODEV

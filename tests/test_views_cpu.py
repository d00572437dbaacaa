"""The view and placement variants of util.py (util.VARIANTS), checked without a GPU.

tests/test_gpu_views.py renders every row of the kernel pick table under each variant and compares it with the oracle.  For
that comparison to mean something, three things must hold, and they are checked here:

  1. the oracle (oracle/pt_oracle.c) is the compiled reference's frame on these inputs as well, bit for bit -- sphere rows
     against the reference as shipped, mesh rows against its revived mesh scan (as tests/test_oracle_ref.py does for the
     configurations);
  2. each variant does what its name claims, at the rows' image size: the tile cones, frames and distances that the
     kernels' conservative rules (pt_filter.h: tile_cone_reaches_ball; rt_hip_shim.hip: launch_prepare and the margins it
     forms) depend on really reach the edge the variant is named for;
  3. the pick (rt_hip_kernel_for_class, the table behind the C-ABI) does not move: every row keeps its kernel under every
     variant, except the pairs listed in PICK_MOVES, whose geometry legitimately changes the scene's class.
"""
import ctypes as C

import numpy as np
import pytest

from conftest import SEED
from test_gpu_parity import PICK_ROWS, _PW, _WP
from test_pick_table import SceneClass
from util import (FAR_OFFSET, PLACEMENTS, VARIANTS, VIEWS, camera_arrays, class_scene, mesh_ball, pick_moves, scene_parts,
                  view_variant)

TILE = 8
ROW_IDS = [f"{k}:{i}:{'+'.join(f'{a}={b}' for a, b in c.items())}{':fault%d' % f if f else ''}" for c, i, f, k in PICK_ROWS]

def near_R(sc):
    """launch_prepare's near_R: 1.5 (|camera| + reach) + 1, reach over the spheres of radius < 1000 and every vertex"""
    objs, meshes = scene_parts(sc)
    reach = max([np.linalg.norm(o["center"]) + abs(o["radius"]) for o in objs if abs(o["radius"]) < 1000] +
                [float(np.sqrt((m["vertices"][:, :3] ** 2).sum(axis=1)).max()) for m in meshes] + [0.0])
    return 1.5 * (np.linalg.norm(camera_arrays(sc.camera)[0]) + reach) + 1.0


def tile_cones(sc):
    """[tiles_y, tiles_x] half-angle of each tile's cone of camera rays as tile_cone_reaches_ball bounds it: the angle between
    the normalised sum a of the four corner vectors w = pos - (llc + H u + V v), u in [tx0, tx0 + 8] / (W - 1), v likewise,
    and the farthest corner (exact fp64 here, not the kernel's seeds); -> (theta, a)"""
    pos, H, V, llc = camera_arrays(sc.camera)
    w, h = sc.width, sc.height
    tx, ty = (w + TILE - 1) // TILE, (h + TILE - 1) // TILE
    u = np.arange(tx + 1) * TILE / (w - 1.0)
    v = np.arange(ty + 1) * TILE / (h - 1.0)
    W = pos - (llc + H * u[None, :, None] + V * v[:, None, None])           # [ty + 1, tx + 1, 3]
    Wn = W / np.linalg.norm(W, axis=2, keepdims=True)
    corners = [Wn[:-1, :-1], Wn[:-1, 1:], Wn[1:, :-1], Wn[1:, 1:]]
    raw = [W[:-1, :-1], W[:-1, 1:], W[1:, :-1], W[1:, 1:]]
    a = sum(raw)
    a = a / np.linalg.norm(a, axis=2, keepdims=True)
    cos_t = np.min([(a * c).sum(axis=2) for c in corners], axis=0)
    return np.arccos(np.clip(cos_t, -1, 1)), a


def frame_coords(sc):
    """pos - llc = H x + V y + n z with n the frame's unit normal -> (x, y, z)"""
    pos, H, V, llc = camera_arrays(sc.camera)
    n = np.cross(H, V)
    n /= np.linalg.norm(n)
    return np.linalg.solve(np.stack([H, V, n], axis=1), pos - llc)


# ---- 1. the oracle is the compiled reference's frame under every variant ---------------------------------------------------

SPHERE_ROWS = []
for _c, _i, _f, _k in PICK_ROWS:
    if not _c.get("tris") and _c.get("depth", 5) == 5 and (_c, _i) not in [(c, i) for c, i, _ in SPHERE_ROWS]:
        SPHERE_ROWS.append((_c, _i, _k))
MESH_ROWS = [(dict(n_packed=4, tris=40, mesh_chk=True), "path"), (dict(n_packed=4, tris=400, round_mesh=True), "path"),
             (dict(n_packed=4, tris=40), "whitted")]


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("cls,integrator,kernel", SPHERE_ROWS, ids=[f"{k}:{i}" for c, i, k in SPHERE_ROWS])
def test_oracle_is_the_reference_under_the_variant_sphere_rows(pt, ref, cls, integrator, kernel, variant):
    sc = view_variant(class_scene(**cls), variant)
    m1, b1, s1 = pt.render_pixels(sc, SEED, integrator=integrator)
    m2, b2, s2 = ref(sc.max_depth).render_pixels(sc, SEED, integrator=integrator)
    assert np.array_equal(m1, m2), f"{kernel} {variant}: fp64 means differ from the compiled reference"
    assert np.array_equal(b1, b2)
    assert (s1["rays"], s1["tests"]) == (s2["rays"], s2["tests"])
    assert m1.any()


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("cls,integrator", MESH_ROWS, ids=[f"{'+'.join(f'{a}={b}' for a, b in c.items())}:{i}" for c, i in MESH_ROWS])
def test_oracle_is_the_reference_under_the_variant_mesh_rows(pt, ref_mesh, cls, integrator, variant):
    sc = view_variant(class_scene(**cls), variant)
    m1, b1, s1 = pt.render_pixels(sc, SEED, integrator=integrator)
    m2, b2, s2 = ref_mesh(sc.max_depth).render_pixels(sc, SEED, integrator=integrator)
    assert np.array_equal(m1, m2), f"{cls} {variant}: fp64 means differ from the compiled reference + revived mesh scan"
    assert np.array_equal(b1, b2)
    assert (s1["rays"], s1["tests"]) == (s2["rays"], s2["tests"])
    assert s1["tests"] == s1["casts"] * (sc.n_objects + sc.n_triangles)


# ---- 2. the variants reach their edges ------------------------------------------------------------------------------------

@pytest.mark.parametrize("cls,integrator,faults,kernel", PICK_ROWS, ids=ROW_IDS)
def test_the_variants_reach_their_edges(cls, integrator, faults, kernel):
    base = class_scene(**cls)
    objs0, meshes0 = scene_parts(base)
    pos0, H0, V0, llc0 = camera_arrays(base.camera)
    assert np.linalg.det(np.stack([H0, V0, pos0 - llc0])) > 0, "init_camera's frame is the positive orientation"
    for variant in VARIANTS:
        sc = view_variant(base, variant)
        what = f"{kernel} {variant}"
        assert (sc.width, sc.height, sc.samples, sc.max_depth) == (base.width, base.height, base.samples, base.max_depth)
        assert (sc.n_objects, sc.n_meshes, sc.n_triangles) == (base.n_objects, base.n_meshes, base.n_triangles)
        objs, meshes = scene_parts(sc)
        pos, H, V, llc = camera_arrays(sc.camera)
        assert np.isfinite(np.concatenate([pos, H, V, llc])).all(), what
        assert near_R(sc) < 1e15, what
        # the eye is off its frame's plane: no (u, v) of a jittered sample gives a zero direction
        x, y, z = frame_coords(sc)
        assert abs(z) >= 1e-3 * (1 - 1e-9) * (1e-3 if variant == "tiny" else 1.0), what
        theta, _ = tile_cones(sc)
        if variant in VIEWS:   # the geometry is the row's own, bit for bit
            assert [(o["center"], o["radius"]) for o in objs] == [(o["center"], o["radius"]) for o in objs0], what
            assert all(np.array_equal(m["vertices"], m0["vertices"]) for m, m0 in zip(meshes, meshes0)), what
        if variant == "wide":
            assert theta.max() > np.pi / 2, f"{what}: no tile cone wider than 90 degrees ({np.degrees(theta.max())})"
        elif variant == "telephoto":
            assert theta.max() < 1e-5, f"{what}: a tile cone of {theta.max()} rad"
            if meshes:   # aimed past the triangles' ball: some tile's cone misses it by more than the kernel's margins
                c, R = mesh_ball(meshes)
                L = c - pos
                _, a = tile_cones(sc)
                off = np.arccos(np.clip((a @ L) / np.linalg.norm(L), -1, 1)) - theta - np.arcsin(R / np.linalg.norm(L))
                assert off.min() > 1e-2, f"{what}: some tile may see the mesh's ball"
            else:        # the first packed sphere's edge is in view: some tiles see it and some do not
                c, R = np.array(objs[8]["center"]), objs[8]["radius"]
                L = c - pos
                _, a = tile_cones(sc)
                ang = np.arccos(np.clip((a @ L) / np.linalg.norm(L), -1, 1)) - np.arcsin(R / np.linalg.norm(L))
                assert (ang < -theta).any() and (ang > theta).any(), what
        elif variant == "sheared":
            assert np.linalg.det(np.stack([H, V, pos - llc])) < 0, f"{what}: not mirrored"
            assert abs(H @ V) > 0.1 * np.linalg.norm(H) * np.linalg.norm(V), f"{what}: H and V orthogonal"
            assert not (0 <= x <= 1 and 0 <= y <= 1), f"{what}: the principal ray lies inside the frame"
            assert abs(np.cross(H0 / np.linalg.norm(H0), H / np.linalg.norm(H)) @ (pos0 - llc0)) > 0, f"{what}: not rolled"
        elif variant == "near_plane":
            assert 0 < x < 1 and 0 < y < 1, f"{what}: the eye is not over the frame"
            assert abs(abs(z) - 1e-3) < 1e-12, what
            assert theta.max() > np.radians(80), what
        elif variant == "steep":
            f = -(pos - llc - H / 2 - V / 2)
            assert abs(f[1]) / np.linalg.norm(f) > 0.999999, f"{what}: not looking straight down"
        elif variant == "inside":
            small = [o for o in objs if o["radius"] < 1000]
            walls = [o for o in objs if 1000 <= o["radius"] < 1e15]
            assert all(np.linalg.norm(pos - o["center"]) > o["radius"] for o in walls), f"{what}: outside the room"
            if meshes:
                c, R = mesh_ball(meshes)
                assert np.linalg.norm(pos - c) < R, f"{what}: outside the mesh's ball"
                if cls.get("round_mesh"):   # inside the tessellated ball itself: within its inscribed radius
                    n_lat = max(2, int(round((cls["tris"] / 4.0) ** 0.5)))
                    assert np.linalg.norm(pos - np.array([2.0, -3.0, 8.0])) < 7.0 * np.cos(np.pi / n_lat) ** 2, what
            if cls.get("refr") and sc.max_depth <= 8:   # inside the glass packed sphere
                assert np.linalg.norm(pos - objs[8]["center"]) < objs[8]["radius"], f"{what}: outside the glass sphere"
            else:                           # among the packed spheres
                assert all(np.linalg.norm(pos - o["center"]) > o["radius"] for o in small), f"{what}: inside a sphere"
            d = pos - llc - H / 2 - V / 2
            assert min(abs(d / np.linalg.norm(d))) > 0.1, f"{what}: aimed along an axis"
        elif variant == "far":
            smallest = min(o["radius"] for o in objs0 if o["radius"] < 1000)
            edges = [np.linalg.norm(m["vertices"][k::3, :3] - m["vertices"][(k + 1) % 3::3, :3], axis=1)
                     for m in meshes0 for k in range(3)]
            bound = 0.25 * max([smallest] + ([float(np.median(np.concatenate(edges)))] if edges else []))
            cs = [np.linalg.norm(o["center"]) for o in objs if o["radius"] < 1000] + \
                 [float(r) for m in meshes for r in np.linalg.norm(m["vertices"][:, :3], axis=1)]
            spacing = min(float(np.spacing(np.float32(c))) for c in cs)
            assert spacing >= bound, f"{what}: fp32 spacing {spacing} at the centres < {bound}"
            assert near_R(sc) < 1e9, what
            assert np.array_equal(pos - np.array(FAR_OFFSET), pos0) or np.allclose(pos - np.array(FAR_OFFSET), pos0, atol=4.0)
        elif variant in ("tiny", "huge"):
            s = 1e-3 if variant == "tiny" else 1e3
            assert np.allclose(pos, pos0 * s) and np.allclose(H, H0 * s) and np.allclose(llc, llc0 * s)
            assert all(np.isclose(o["radius"], o0["radius"] * s) for o, o0 in zip(objs, objs0))
            assert [o["emission"] for o in objs] == [o["emission"] for o in objs0]
            assert [o["color"] for o in objs] == [o["color"] for o in objs0]
    base.free()


# ---- 3. the pick does not move -------------------------------------------------------------------------------------------

def scene_class(sc, integrator, faults):
    """the class rt_hip_scene_create forms of a scene (rt_hip_shim.hip), for one launch of all its samples in one chunk"""
    objs, meshes = scene_parts(sc)
    both = 4 | 8
    flags = [o["flags"] for o in objs] + [m["flags"] for m in meshes]
    wide = any(not (np.linalg.norm(o["center"]) <= 1e17) or not (abs(o["radius"]) <= 1e17) for o in objs)
    rnd = 0
    if meshes:
        v = np.concatenate([m["vertices"][:, :3] for m in meshes])
        lo, hi = v.min(axis=0), v.max(axis=0)
        c, R = mesh_ball(meshes)
        a, b, d = hi - lo
        rnd = int(3.14159265358979 * R * R <= 0.5 * (a * b + b * d + d * a))
    emission = max([abs(e) for o in objs for e in o["emission"]] + [abs(e) for m in meshes for e in m["emission"]] + [0.0])
    return SceneClass(0 if integrator == "path" else 1, len(objs), len(meshes), sc.n_triangles,
                      int(any(f & 16 for f in flags)), int(any(f & 8 for f in flags)), int(any(f & both == both for f in flags)),
                      int(wide), rnd, sc.samples, sc.max_depth, int(not faults & _PW), int(not faults & _WP), emission)


@pytest.mark.parametrize("cls,integrator,faults,kernel", PICK_ROWS, ids=ROW_IDS)
def test_the_pick_does_not_move_under_any_variant(cls, integrator, faults, kernel):
    from rt_amd import abi
    shim = abi.load_shim()
    base = class_scene(**cls)
    own = shim.rt_hip_kernel_for_class(C.byref(scene_class(base, integrator, faults))).decode()
    assert own == kernel or cls.get("depth") == 30   # (those take their row through the launch's facts, as in the row test)
    moved = []
    for variant in VARIANTS:
        got = shim.rt_hip_kernel_for_class(C.byref(scene_class(view_variant(base, variant), integrator, faults))).decode()
        if pick_moves(cls, kernel, variant):
            assert got != own, f"{kernel} {variant}: listed in PICK_MOVES but keeps its row"
            moved.append(variant)
        else:
            assert got == own, f"{kernel} {variant}: the pick moved to {got}"
    assert moved == (["tiny"] if cls.get("wide") else []), moved
    base.free()


def test_far_offset_is_what_the_comment_states():
    """|FAR_OFFSET| lies in [2^24, 2^25): fp32 spacing 2 there, with room for the rows' extent on either side"""
    r = float(np.linalg.norm(FAR_OFFSET))
    assert 2.0 ** 24 + 100 < r < 2.0 ** 25 - 100
    assert np.spacing(np.float32(r)) == 2.0
    assert len(set(np.sign(FAR_OFFSET))) == 2 and PLACEMENTS == ("far", "tiny", "huge")

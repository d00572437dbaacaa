"""The CPU expectation of a ray query (include/rt_hip.h, rt_hip_query_rays), from the compiled reference alone: get_camera_ray
(camera_ray) for (u, v) rays, the contract's vec3_normalize in numpy fp64 (m = sqrt((x*x + y*y) + z*z), d * (1.0 / m): the same
IEEE operations), the validity rule, one intersect() -- the reference's scan with its mesh block revived (intersect_mesh_scene:
the winner's own t, point, normal and id) -- and the t_max rule.  prim is the lowest global triangle index of the winning mesh
whose compiled intersect_triangle gives the winner's t, bary that call's u, v (read off as texture coordinates of the corners
(0, 0), (1, 0), (0, 1): 0 * w + 1 * u + 0 * v is u exactly, but for u = -0.0, which the sum turns into +0.0).  Also the ray sets the GPU tests query, built so that the reference's
answers are non-trivial (tests/test_query_cpu.py asserts that).
"""
import numpy as np

import util

NO_HIT = 0xFFFFFFFF
BAND = 2.0 ** -13
FIELDS = ("status", "t", "object", "prim", "point", "normal", "bary", "ray")


def normalize(d):
    """vec3_normalize (vector.h:53-58) of every row, fp64, unfused"""
    d = np.asarray(d, dtype=np.float64)
    with np.errstate(all="ignore"):
        m = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        return d * (1.0 / m)[:, None]


def valid_mask(rays, t_max):
    with np.errstate(all="ignore"):
        d = rays[:, 3:]
        dd = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        ok = np.isfinite(rays).all(axis=1) & (np.abs(dd - 1.0) <= BAND)
    return ok & ~np.isnan(t_max)


def _mesh_vertices(sc):
    """per mesh: (first global triangle index, vertices [3 n, 5])"""
    _, meshes = util.scene_parts(sc)
    out, first = [], 0
    for m in meshes:
        out.append((first, m["vertices"]))
        first += len(m["vertices"]) // 3
    return out


def _winner_triangle(ref, ray, first, verts, t_win):
    """the lowest triangle of the mesh whose compiled intersect_triangle gives t_win -> (global index, u, v).  numpy only narrows
    the search (Moeller-Trumbore in fp64, every triangle within 1e-6 relative of t_win); the compiled call decides"""
    v0, v1, v2 = verts[0::3, :3], verts[1::3, :3], verts[2::3, :3]
    o, d = ray[:3], ray[3:]
    with np.errstate(all="ignore"):
        e1, e2 = v1 - v0, v2 - v0
        h = np.cross(d, e2)
        a = (e1 * h).sum(axis=1)
        s = o - v0
        q = np.cross(s, e1)
        t = (e2 * q).sum(axis=1) / a
        near = np.nonzero(np.abs(t - t_win) <= 1e-6 * abs(t_win))[0]
    for k in near:
        v15 = np.zeros(15)
        v15[0:3], v15[5:8], v15[10:13] = v0[k], v1[k], v2[k]
        v15[8], v15[14] = 1.0, 1.0   # tex (0, 0), (1, 0), (0, 1): the interpolation returns the barycentrics
        ok, out = ref.intersect_triangle(ray, v15)
        if ok and out[0] == t_win:
            return first + int(k), out[1], out[2]
    raise AssertionError("no triangle of the winning mesh reproduces the winner's t")


def expected(ref, sc, rays=None, uv=None, camera=None, t_max=None, normalize_dirs=False, extra=None):
    """ref: an oracle_py.RefMeshOracle.  rays [n, 6], or uv [n, 2] with `camera` (None: the scene's).  -> dict of arrays as the
    device buffers hold them.  extra: a dict that receives u_win / v_win, the winner's own texture coordinates [n]"""
    if uv is not None:
        cam = camera if camera is not None else sc.camera
        rays = np.array([ref.camera_ray(cam, float(u), float(v)) for u, v in np.asarray(uv, dtype=np.float64).reshape(-1, 2)]).reshape(-1, 6)
    rays = np.array(rays, dtype=np.float64).reshape(-1, 6)
    n = len(rays)
    if normalize_dirs:
        rays[:, 3:] = normalize(rays[:, 3:])
    t_max = np.full(n, np.finfo(np.float64).max) if t_max is None else np.asarray(t_max, dtype=np.float64).reshape(n)
    ok = valid_mask(rays, t_max)
    out = dict(status=np.where(ok, 0, 2).astype(np.uint32), t=np.full(n, np.inf), object=np.full(n, NO_HIT, np.uint32),
               prim=np.full(n, NO_HIT, np.uint32), point=np.zeros((n, 3)), normal=np.zeros((n, 3)), bary=np.zeros((n, 2)), ray=rays)
    uw, vw = np.zeros(n), np.zeros(n)
    meshes = _mesh_vertices(sc)
    for i in np.nonzero(ok)[0]:
        hit = ref.intersect_mesh_scene(rays[i], sc)
        if not hit["hit"] or not (hit["min_t"] < t_max[i]):
            continue
        out["status"][i], out["t"][i], out["object"][i] = 1, hit["min_t"], hit["id"]
        out["point"][i], out["normal"][i] = hit["point"], hit["normal"]
        uw[i], vw[i] = hit["u_win"], hit["v_win"]
        if hit["id"] >= sc.n_objects:
            first, verts = meshes[hit["id"] - sc.n_objects]
            out["prim"][i], out["bary"][i, 0], out["bary"][i, 1] = _winner_triangle(ref, rays[i], first, verts, hit["min_t"])
    if extra is not None:
        extra["u_win"], extra["v_win"] = uw, vw
    return out


def mismatch(got, exp, fields=FIELDS):
    """'' when every array of `got` equals `exp`'s bit for bit, else the first difference"""
    for f in fields:
        g, e = np.ascontiguousarray(got[f]), np.ascontiguousarray(exp[f])
        g = g.view(np.uint32) if g.dtype == np.int32 else g
        if g.shape != e.shape:
            return f"{f}: shape {g.shape} != {e.shape}"
        gb = g.view(np.uint64 if g.dtype == np.float64 else np.uint32)
        eb = e.astype(g.dtype).view(gb.dtype)
        bad = np.nonzero((gb != eb).reshape(len(g), -1).any(axis=1))[0]
        if len(bad):
            k = int(bad[0])
            return f"{f}: {len(bad)} of {len(g)} rays differ, first ray {k}: got {g[k]!r}, expected {e[k]!r}"
    return ""


# ---- the scenes and ray sets of tests/test_gpu_query.py ---------------------------------------------------------------------
# one scene per query form (pt_query_pick: the five geometric forms of the AOV list; the memory form at 257 spheres, the
# smallest count whose geometry + materials leave the 24 KB staging budget: 96 bytes per sphere), then coincident triangles,
# walls met from inside a room, and a lopsided hierarchy
SCENES = {
    "rays": ("pt_query_rays", lambda: util.class_scene(n_packed=4)),
    "tri": ("pt_query_rays_tri", lambda: util.class_scene(n_packed=4, tris=40)),
    "big": ("pt_query_rays_big", lambda: util.class_scene(n_packed=4, wide=True)),
    "tri_big": ("pt_query_rays_tri_big", lambda: util.class_scene(n_packed=4, tris=400, open_back=True)),
    "mem": ("pt_query_rays_mem", lambda: util.class_scene(n_packed=249, tris=60)),
    "soup": ("pt_query_rays_tri", lambda: util.mesh_soup_scene(duplicates=True)),
    "convex": (None, lambda: util.convex_body_scene(7)[0]),
    "walls": (None, lambda: util.walls_scene(3)),
    "lopsided": ("pt_query_rays_tri_big", lambda: util.lopsided_mesh_scene(11)),
}
OPEN_SCENES = ("soup", "convex")
N_RAYS = 2048


def ray_set(sc, n=N_RAYS, seed=20260101):
    """n rays for scene `sc`: origins at free points (outside every sphere) spread over the scene, half the directions aimed at
    points on primitives, half uniform over the sphere; unit to rounding.  Fixed seed."""
    rng = np.random.default_rng(seed)
    objs, meshes = util.scene_parts(sc)
    small = [o for o in objs if o["radius"] < 1000]
    pts = [np.array(o["center"]) for o in small] + [m["vertices"][:, :3].mean(axis=0) for m in meshes]
    centre = np.mean(pts, axis=0) if pts else np.zeros(3)
    spread = max(4.0, float(np.max([np.linalg.norm(p - centre) for p in pts])) if pts else 4.0)
    anchors = [util.free_point(objs, centre + rng.uniform(-1, 1, 3) * 0.6 * spread, clearance=0.25) for _ in range(16)]
    origins = np.array([anchors[k % 16] for k in range(n)]) + rng.uniform(-0.2, 0.2, (n, 3))
    dirs = rng.normal(size=(n, 3))
    tri_v = np.concatenate([m["vertices"][:, :3] for m in meshes]).reshape(-1, 3, 3) if meshes else None
    for k in range(0, n, 2):   # aimed: alternately at a triangle (where there are any) and at a sphere of ordinary size
        if tri_v is not None and (k // 2) % 2 == 0:
            b = rng.dirichlet((1.0, 1.0, 1.0))
            target = (tri_v[rng.integers(len(tri_v))] * b[:, None]).sum(axis=0)
        elif small:
            o = small[rng.integers(len(small))]
            v = rng.normal(size=3)
            target = np.array(o["center"]) + 0.7 * o["radius"] * v / np.linalg.norm(v)
        else:
            continue
        dirs[k] = target - origins[k]
    dirs /= np.sqrt((dirs * dirs).sum(axis=1))[:, None]
    return np.concatenate([origins, dirs], axis=1)

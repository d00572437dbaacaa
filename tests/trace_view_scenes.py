"""The scene classes, pixel lists and ray lists with which the ten path-tracing query kernels -- pt_trace_rays[_big|_tri|_tri_big|_mem]
and pt_trace_pixels[_big|_tri|_tri_big|_mem] -- are compared with the compiled reference under every view and placement variant
(util.VARIANTS): tests/test_gpu_trace_views.py runs them on the device, tests/test_trace_views_cpu.py shows from the oracles alone
what they reach.  No tests in here.

Every form is instantiated <REFRACT = true, CHECKER = true>, so every form carries every material's code; TRACE_VIEW_CLASSES puts
every material on every form:

  form        glass sphere   glass2 sphere   glass mesh      checkered wall   checkered mesh
  plain       all_sph        all_sph         -               all_sph          -
  _big        big_mat        -               -               big_mat          -
  _tri        tri_chk        -               tri_glass       tri_glass, tri_plain   tri_chk, tri_plain
  _tri_big    -              tri_big_chk     tri_big_glass   -                tri_big_chk
  _mem        mem_mat, mem_sph   -           -               mem_sph          mem_mat

(glass2: M_REFLECTION | M_REFRACTION on one sphere.)  tri_plain is the one class without M_REFRACTION: its samples are held to the
bar without the refraction term, 2^-40 |ref| (trace_expected.value_bar), and it has a checkered wall AND a checkered mesh, so a
checkered sphere is hit by rays that passed a triangle -- the reference then reads the last passing triangle's hit.u / hit.v for
the sphere (trace_step's TriLast route).
"""
import numpy as np

import refine_expected as R
import trace_expected as T
import util

W, H, DEPTH = 31, 23, 4          # ragged against the 8 x 8 tiles; depth <= 8 so that view_variant("inside") enters the glass sphere
PIXEL_S, PIXEL_S0 = 5, 3         # trace_pixels: samples 3 .. 7
RAY_S = 3                        # trace_rays: samples 0 .. 2
SEED = 20260505
N_UV, N_SET = 33, 32

# (name, class_scene kwargs, trace form, pixel form, glass: the scene has M_REFRACTION -- which bar its samples are held to)
TRACE_VIEW_CLASSES = [
    ("all_sph", dict(n_packed=4, chk=True, refr=True, glass2=True), "pt_trace_rays", "pt_trace_pixels", True),
    ("big_mat", dict(n_packed=4, wide=True, chk=True, refr=True), "pt_trace_rays_big", "pt_trace_pixels_big", True),
    ("tri_chk", dict(n_packed=4, tris=40, mesh_chk=True, refr=True), "pt_trace_rays_tri", "pt_trace_pixels_tri", True),
    ("tri_glass", dict(n_packed=4, tris=40, mesh_refr=True, chk=True), "pt_trace_rays_tri", "pt_trace_pixels_tri", True),
    ("tri_plain", dict(n_packed=4, tris=40, mesh_chk=True, chk=True), "pt_trace_rays_tri", "pt_trace_pixels_tri", False),
    ("tri_big_glass", dict(n_packed=4, tris=400, mesh_refr=True, open_back=True), "pt_trace_rays_tri_big", "pt_trace_pixels_tri_big", True),
    ("tri_big_chk", dict(n_packed=4, tris=400, mesh_chk=True, glass2=True), "pt_trace_rays_tri_big", "pt_trace_pixels_tri_big", True),
    # 8 + 249 = 257 spheres: the smallest count beyond the staging budget (pt_geom_in_lds: 96 bytes per sphere, 24 KB)
    ("mem_mat", dict(n_packed=249, tris=60, mesh_chk=True, refr=True), "pt_trace_rays_mem", "pt_trace_pixels_mem", True),
    # the memory form with TRIS = true and n_tri = 0 ("triangles (if any)")
    ("mem_sph", dict(n_packed=300, chk=True, refr=True), "pt_trace_rays_mem", "pt_trace_pixels_mem", True),
]
CLASS_NAMES = [c[0] for c in TRACE_VIEW_CLASSES]
CLASSES = {c[0]: c for c in TRACE_VIEW_CLASSES}
FORMS = sorted({c[2] for c in TRACE_VIEW_CLASSES}) + sorted({c[3] for c in TRACE_VIEW_CLASSES})

# (class, variant) -> (trace form, pixel form) the launches take instead of the class's own, and why
TRACE_MOVES = {
    # the floor of radius 1e19 is the only thing that makes big_mat wide_range (a centre or radius beyond 1e17); scaled by 1e-3 it
    # is 1e16, and with 13 spheres and no triangles pt_filter_in_lds holds: the staged-filter forms take the scene.
    ("big_mat", "tiny"): ("pt_trace_rays", "pt_trace_pixels"),
    # not listed, for these reasons: the _tri_big classes are _big through their 400 triangles (> 256 filter entries), not through
    # a range; the _mem classes through 257 / 308 spheres, which pt_trace_pick asks first; huge and far make nothing wide (walls
    # of 1e4 x 1e3 = 1e7, centres 2e7 out), and the floor of 1e19 x 1e3 = 1e22 stays wide; a camera changes no scene class
}


def forms_under(name, variant):
    """-> (trace form, pixel form) of class `name` under `variant`"""
    return TRACE_MOVES.get((name, variant), CLASSES[name][2:4])


def picked_forms(sc):
    """pt_trace_pick (pt_kernel.hip) restated from the scene's facts: _mem when sphere geometry + materials are beyond the 24 KB
    staging budget (pt_geom_in_lds: 4 + 8 doubles per sphere, 8 per mesh); else the staged-filter forms when there are at most 256
    spheres + triangles and no centre or radius beyond 1e17 (pt_filter_in_lds); else the _big forms; _tri with any triangle"""
    objs, _ = util.scene_parts(sc)
    wide = any(not (abs(x) <= 1e17) for o in objs for x in o["center"] + (o["radius"],))
    geom_in_lds = (4 * sc.n_objects + 8 * (sc.n_objects + sc.n_meshes)) * 8 <= 24 * 1024
    if not geom_in_lds:
        tail = "_mem"
    elif sc.n_objects + sc.n_triangles <= 256 and not wide:
        tail = "_tri" if sc.n_triangles else ""
    else:
        tail = "_tri_big" if sc.n_triangles else "_big"
    return "pt_trace_rays" + tail, "pt_trace_pixels" + tail


def scene_under(name, variant=None):
    """the scene of class `name` at W x H, depth DEPTH, under `variant` (None: the class's own camera and placement)"""
    base = util.class_scene(depth=DEPTH, width=W, height=H, **CLASSES[name][1])
    if base.n_meshes:
        # class_scene gives every triangle the texture coordinates (0, 0), (1, 0), (0, 1): the last passing triangle's and the
        # winner's are then the same six numbers, and a kernel that blends the wrong triangle's goes unnoticed.  Random ones here.
        objs, meshes = util.scene_parts(base)
        rng = np.random.default_rng(20260507)
        for m in meshes:
            m["vertices"][:, 3:5] = rng.random((len(m["vertices"]), 2))
        textured = util._rebuild(base, objs, meshes, base.camera)
        base.free()
        base = textured
    if variant is None:
        return base
    sc = util.view_variant(base, variant)
    base.free()
    return sc


def has_refraction(sc):
    from rt_amd import abi
    objs, meshes = util.scene_parts(sc)
    return any(m["flags"] & abi.M_REFRACTION for m in objs + meshes)


def pixel_list():
    return R.pixel_list(W, H)


def uv_points():
    """N_UV points of the frame's (u, v): the four corners, the middle, eight outside [0, 1] (every side and every corner of the
    frame passed), the rest inside"""
    rng = np.random.default_rng(20260506)
    fixed = [(0.0, 0.0), (1.0, 0.0), (0.0, 1.0), (1.0, 1.0), (0.5, 0.5),
             (-0.2, 0.5), (1.2, 0.5), (0.5, -0.2), (0.5, 1.2), (-0.1, -0.15), (1.15, -0.1), (-0.15, 1.1), (1.1, 1.2)]
    uv = np.concatenate([np.array(fixed), rng.uniform(0.0, 1.0, (N_UV - len(fixed), 2))])
    assert uv.shape == (N_UV, 2)
    return uv


def _first_t(objs, tri_v, o, d):
    """fp64 numpy: (nearest sphere t or inf, t of every triangle or inf) of the ray (o, d), t > 1e-9 -- only to CHOOSE rays"""
    c, r = np.array([ob["center"] for ob in objs]), np.array([ob["radius"] for ob in objs])
    with np.errstate(all="ignore"):
        L = c - o
        tca = L @ d
        d2 = (L * L).sum(axis=1) - tca * tca
        thc = np.sqrt(r * r - d2)
        t0, t1 = tca - thc, tca + thc
        ts = np.where(t0 > 1e-9, t0, np.where(t1 > 1e-9, t1, np.inf))
        ts = np.where(d2 > r * r, np.inf, ts)
        tt = np.full(0, np.inf)
        if tri_v is not None:
            v0, e1, e2 = tri_v[:, 0], tri_v[:, 1] - tri_v[:, 0], tri_v[:, 2] - tri_v[:, 0]
            h = np.cross(d, e2)
            a = (e1 * h).sum(axis=1)
            sv = o - v0
            u = (sv * h).sum(axis=1) / a
            q = np.cross(sv, e1)
            v = (q @ d) / a
            t = (e2 * q).sum(axis=1) / a
            tt = np.where((np.abs(a) > 1e-9) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > 1e-9), t, np.inf)
    return float(ts.min()), tt


def aimed_rays(base):
    """-> (origins, targets) of a few rays that the random sets cannot be counted on to hold, chosen on the class's own geometry:
    two rays at every sphere with M_REFRACTION, from free points 1.5 radii off its centre (in a room of 257 spheres no random ray's
    first hit is the one glass sphere); and, where a mesh is checkered, up to four rays through TWO of its triangles, the nearer
    one -- the hit -- of lower index than the farther: the reference then reads the farther one's hit.u / hit.v (the last
    passing triangle's; trace_step's TriLast route), and the rays are kept only where that reading and the winner's own texture
    coordinates give different checker factors"""
    from rt_amd import abi
    objs, meshes = util.scene_parts(base)
    finite = [ob for ob in objs if ob["radius"] < 1e15]
    tri_v = np.concatenate([m["vertices"][:, :3] for m in meshes]).reshape(-1, 3, 3) if meshes else None
    o_out, q_out = [], []
    for ob in objs:
        if ob["flags"] & abi.M_REFRACTION:
            c, r = np.array(ob["center"]), ob["radius"]
            for side in ((0.6, 0.48, 0.64), (-0.64, 0.6, 0.48)):
                o = util.free_point(finite, c + 1.5 * r * np.array(side), clearance=0.05)
                o_out.append(o)
                q_out.append(o - (c + 0.3 * r * np.array(side[::-1]) - o) / np.linalg.norm(c + 0.3 * r * np.array(side[::-1]) - o))
    if tri_v is not None and any(m["flags"] & abi.M_CHECKERED for m in meshes) and len(meshes) == 1:
        tex = meshes[0]["vertices"][:, 3:5].reshape(-1, 3, 2)
        cen = tri_v.mean(axis=1)
        c, r = np.array([ob["center"] for ob in finite]), np.array([ob["radius"] for ob in finite])

        def checker_bit(tx, u, v):
            tu, tv = (tx[0, 0] * (1 - u - v) + tx[1, 0] * u) + tx[2, 0] * v, (tx[0, 1] * (1 - u - v) + tx[1, 1] * u) + tx[2, 1] * v
            return bool((np.fmod(tu * 100000.0, 1.0) > 0.5) ^ (np.fmod(tv * 100000.0, 1.0) < 0.5))
        found = 0
        for a in range(len(cen)):
            for b in range(a + 1, len(cen)):
                gap = np.linalg.norm(cen[b] - cen[a])
                if found == 4 or not 0.05 < gap < 12.0:
                    continue
                d = (cen[b] - cen[a]) / gap
                o = cen[a] - 0.5 * d
                if not (np.sqrt(((c - o) ** 2).sum(axis=1)) > r + 0.05).all():
                    continue
                t_sph, tt = _first_t(finite, tri_v, o, d)
                passing = np.flatnonzero(np.isfinite(tt))
                if len(passing) < 2 or not tt.min() < t_sph or passing[-1] == int(tt.argmin()):
                    continue
                # the two readings must give different checker factors: the last passing triangle's barycentrics with its own
                # texture coordinates (the reference) and with the winner's (the mistake to be noticed)
                win, last = int(tt.argmin()), int(passing[-1])
                e1, e2, sv = tri_v[last, 1] - tri_v[last, 0], tri_v[last, 2] - tri_v[last, 0], o - tri_v[last, 0]
                h = np.cross(d, e2)
                u, v = (sv @ h) / (e1 @ h), (np.cross(sv, e1) @ d) / (e1 @ h)
                if checker_bit(tex[last], u, v) != checker_bit(tex[win], u, v):
                    o_out.append(o)
                    q_out.append(o - d)
                    found += 1
                    break       # the next ray through another nearer triangle
    return np.array(o_out).reshape(-1, 3), np.array(q_out).reshape(-1, 3)


def ray_list(sc, name, variant):
    """`sc` = scene_under(name, variant) -> (origins, targets) of the rays for trace_expected.reference_samples (ray i = (o,
    vec3_normalize(o - q))): first N_UV camera rays of the scene's own camera at uv_points() -- the target is the frame point
    llc + H u + V v, so the ray is get_camera_ray's to rounding --, then N_SET rays of trace_expected.ray_set, then aimed_rays:
    65 to 73 rays, more than one workgroup of 64.  The last two sets depend on the geometry alone and are built with lengths of
    the class's own scale (clearances of 0.25, spheres of radius < 1000 as the ones to aim at), so they are built on the class's
    own scene and moved as util.view_variant moves the geometry: o -> s o + off under a placement, as they are under a camera"""
    pos, Hv, Vv, llc = util.camera_arrays(sc.camera)
    uv = uv_points()
    o_cam = np.repeat(pos[None, :], N_UV, axis=0)
    q_cam = llc[None, :] + Hv[None, :] * uv[:, :1] + Vv[None, :] * uv[:, 1:]
    base = scene_under(name)
    o, q = T.ray_set(base, N_SET, open_back=bool(CLASSES[name][1].get("open_back")))
    o2, q2 = aimed_rays(base)
    base.free()
    o, q = np.concatenate([o, o2]), np.concatenate([q, q2])
    if variant in util.PLACEMENTS:
        s, off = util.SCALES.get(variant, 1.0), (np.array(util.FAR_OFFSET) if variant == "far" else np.zeros(3))
        o, q = o * s + off, q * s + off
    return np.concatenate([o_cam, o]), np.concatenate([q_cam, q])


def first_hits(ref, pt, sc, rays, streams, seed):
    """what the FIRST scan of each sample's ray meets, from the compiled reference's own scan (a cheap witness: paths meet more).
    rays [n, 6]; streams [n] of (stream index, sample).  -> dict of arrays [n]: hit, flags (of the object hit; 0 for a miss),
    tri (a triangle is the winner), stale (the ray passed a triangle and hit.u / hit.v are not the winner's own), on (the
    checker's bit for the u, v the reference reads: factor 0.7 when set, 0.3 when not), alive (the roulette draw -- the stream's
    third -- lets the path go on: the material's code runs)"""
    n = len(rays)
    out = dict(hit=np.zeros(n, bool), flags=np.zeros(n, np.int64), tri=np.zeros(n, bool), stale=np.zeros(n, bool),
               on=np.zeros(n, bool), alive=np.zeros(n, bool), id=np.full(n, -1, np.int64))
    for i in range(n):
        h = ref.intersect_mesh_scene(rays[i], sc)
        if not h["hit"]:
            continue
        k = h["id"]
        m = sc.objects[k] if k < sc.n_objects else sc.meshes[k - sc.n_objects]
        out["hit"][i], out["flags"][i], out["tri"][i], out["id"][i] = True, int(m.flags), k >= sc.n_objects, k
        out["stale"][i] = (h["u"], h["v"]) != (h["u_win"], h["v_win"])
        out["on"][i] = (np.fmod(h["u"] * 100000, 1.0) > 0.5) ^ (np.fmod(h["v"] * 100000, 1.0) < 0.5)
        color = m.color.tuple()
        out["alive"][i] = pt.random_doubles(seed, int(streams[i][0]), int(streams[i][1]), 3)[2] < max(color)
    return out


def pixel_sample_rays(ref, pt, sc, pixels, S, s0, seed):
    """render()'s camera rays of samples s0 .. s0 + S - 1 of the valid entries of `pixels` -> (rays [m, 6], streams [m])"""
    w, h = sc.width, sc.height
    rays, streams = [], []
    for p in sorted(set(int(p) for p in pixels if p < w * h)):
        for s in range(s0, s0 + S):
            r = pt.random_doubles(seed, p, s, 2)
            rays.append(ref.camera_ray(sc.camera, (p % w + r[0]) / (w - 1.0), (p // w + r[1]) / (h - 1.0)))
            streams.append((p, s))
    return np.array(rays), streams

"""Ray sets for the ray queries (rt_hip_query_rays, the five pt_query_rays* kernels) where the conservative skipping rules are
tightest: the packed-fp32 sphere filter and its sign-test form, tri_may_hit32, the hierarchy's slab test and the far_origin switch
(pt_filter.h, pt_intersect.h).  Plain numpy, fixed seeds; tests/test_query_edges_cpu.py shows on the compiled reference alone what
each set reaches, tests/test_gpu_query_edges.py compares the kernels with the reference on them, bit for bit.

  (a) variant_rays    each form's scene under every camera and placement of util.VARIANTS: (u, v) rays of the variant's camera and
                      world rays that move and scale with the scene
  (b) shell_rays      origins on a ladder of radii around near_R and around near_R sqrt(0.9999), the far_origin thresholds
  (c) hint_ladder     the origin_radius hints that put those thresholds around a fixed set of origins (fixed_shell)
  (d) grazing_rays    sphere silhouettes, triangle vertices and edges, and points a few ulps to either side of them
  (e) axis_rays       directions with exact zeros (0.0 and -0.0) through vertices, and ladders of consecutive fp32 values across
                      the faces of the mesh's bounding box (where a ray lands exactly on a widened slab plane)
"""
import numpy as np

import query_expected as Q
import util

FORM_SCENES = ("rays", "tri", "big", "tri_big", "mem")         # one scene per query form (Q.SCENES)
HIERARCHY_SCENES = ("tri_big", "mem", "lopsided")                # triangles through the hierarchy
OPEN_BACK = ("tri_big",)                                          # class_scene(open_back=True): camera rays can miss
# (scene, variant) -> the form the launch takes instead of Q.SCENES[scene][0], and why (as util.PICK_MOVES / AOV_MOVES)
QUERY_MOVES = {
    # the floor sphere of radius 1e19 is the only thing that makes `big` wide_range (a centre or radius beyond 1e17); scaled by
    # 1e-3 it is 1e16, and with 13 spheres and no triangles the filter table is staged: the sign-test form takes the scene
    ("big", "tiny"): "pt_query_rays",
    # not listed: `mem` (257 spheres) is beyond the staging budget whatever the range, and tri_big is _big through its 400
    # triangles; huge and far make nothing wide (walls of 1e4 x 1e3 = 1e7, centres 2e7 out); a camera changes no scene class
}
# (open scene, variant) from whose camera no ray leaves the room, and why: the 10 % of missing uv rays is not asked there
SEALED = {
    # the eye at (0, 15, 1e-3) under the ceiling: a ray that clears the ceiling, the floor and the side walls on its way out of the
    # back keeps within 0.08 of the room's axis, and 15 behind the eye all of those pass through the packed sphere of radius 6.6 at
    # (-1.9, 11.1, -15.4).  opening_uv finds none among 9600 candidates (tests/test_query_edges_cpu.py asserts that)
    ("tri_big", "steep"),
}
LADDER_M = (10, 13, 20, 30, 40, 50)
SIGN_TEST_FACTOR = float(np.sqrt(0.9999))     # the sign-test form asks |o'|^2 <= near_R^2 * 0.9999 (pt_filter.h, filter_ray)
UV_GRID = (24, 16)
N_WORLD = 512
N_SHELL = 512
GRAZE_DELTAS = (0.0,) + tuple(s * 2.0 ** -k for k in (10, 20, 30, 40, 50) for s in (1.0, -1.0))
GRAZE_SPHERES, GRAZE_ORIGINS = 32, 4
GRAZE_TRIS = 24            # per mesh ("up to 64": at 102 rays a triangle 64 would be 6.5k rays a mesh; a launch keeps to a few thousand)
GRAZE_SHIFTS = (10, 20, 30, 40, 50)
AXIS_VERTICES = 192
AXIS_DIRS = 6              # directions a vertex (each as fp64 and as fp32)
AXIS_INWARD = 4            # fp32 steps inside the extreme coordinate with which a face ladder starts
AXIS_STEPS_MAX = 512
E24 = 2.0 ** -24


def form_under(name, variant):
    """the query form scene `name` of Q.SCENES takes under `variant` (None: its own camera and place)"""
    return QUERY_MOVES.get((name, variant), Q.SCENES[name][0])


def reach_of(sc):
    """the scene's reach as create_scene forms it (rt_hip_shim.hip): the largest |centre| + |radius| over spheres of radius below
    1000, and |v| over all vertices"""
    objs, meshes = util.scene_parts(sc)
    r = [float(np.linalg.norm(o["center"])) + abs(o["radius"]) for o in objs if abs(o["radius"]) < 1000.0]
    r += [float(np.sqrt((m["vertices"][:, :3] ** 2).sum(axis=1)).max()) for m in meshes if len(m["vertices"])]
    return max(r + [0.0])


def near_R_of(sc, origin_radius=0.0):
    """near_R = 1.5 (origin_radius + reach) + 1 as ray_launch_prepare forms it.  This restatement matches the shim ONLY TO
    ROUNDING (|centre| and |v| are square roots of sums formed in another order there): no set below aims at this value, every
    ladder brackets it from 2^-10 down to 2^-50 on both sides."""
    return 1.5 * (float(origin_radius) + reach_of(sc)) + 1.0


def ladder(R):
    """the 26 radii around R and around R sqrt(0.9999): R (1 + j 2^-m) for m of LADDER_M, j = +-1, and R itself"""
    rel = [0.0] + [j * 2.0 ** -m for m in LADDER_M for j in (1.0, -1.0)]
    return np.array([c * (1.0 + x) for c in (R, R * SIGN_TEST_FACTOR) for x in rel])


def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.sqrt((v * v).sum(axis=-1))[..., None]


def _small(objs, scale=1.0):
    """the spheres of ordinary size (not wall-sized: radius below 1000 in a scene at scale 1)"""
    return [o for o in objs if o["radius"] < 1000 * scale]


def _blocked(small, p0, p1):
    """does a sphere of ordinary size come within 1 % of its radius of the segment p0 -> p1?  (fp64, only to choose origins and
    directions from which the aimed-at primitive can be seen: the reference decides what is hit)"""
    if not small:
        return False
    c, r = np.array([o["center"] for o in small]), np.array([o["radius"] for o in small])
    seg = p1 - p0
    s = np.clip(((c - p0) @ seg) / (seg @ seg), 0.0, 1.0)
    return bool((np.sqrt((((p0 + s[:, None] * seg) - c) ** 2).sum(axis=1)) < 1.01 * r).any())


def _tri_vertices(meshes):
    return np.concatenate([m["vertices"][:, :3] for m in meshes]).reshape(-1, 3, 3) if meshes else None


def _anchors(sc, rng, n=16, clearance=0.25):
    """free points spread over the scene, as Q.ray_set places its origins"""
    objs, meshes = util.scene_parts(sc)
    pts = [np.array(o["center"]) for o in _small(objs)] + [m["vertices"][:, :3].mean(axis=0) for m in meshes]
    centre = np.mean(pts, axis=0)
    spread = max(4.0, float(np.max([np.linalg.norm(p - centre) for p in pts])))
    return [util.free_point(objs, centre + rng.uniform(-1, 1, 3) * 0.6 * spread, clearance=clearance) for _ in range(n)]


def _targets(sc, rng, n):
    """n points on primitives, as Q.ray_set aims: alternately on a triangle (where there are any) and 0.7 r from the centre of a
    sphere of ordinary size"""
    objs, meshes = util.scene_parts(sc)
    small, tri_v = _small(objs), _tri_vertices(meshes)
    out = np.zeros((n, 3))
    for k in range(n):
        if tri_v is not None and (k % 2 == 0 or not small):
            out[k] = (tri_v[rng.integers(len(tri_v))] * rng.dirichlet((1.0, 1.0, 1.0))[:, None]).sum(axis=0)
        else:
            o = small[rng.integers(len(small))]
            out[k] = np.array(o["center"]) + 0.7 * o["radius"] * _unit(rng.normal(size=3))
    return out


# ---- (a) every form under every view and placement -------------------------------------------------------------------------------
def uv_set(seed=20261001):
    """the pixel centres of a 24 x 16 grid, then 64 points of uniform(-0.5, 1.5): inside and around any frame"""
    w, h = UV_GRID
    grid = np.array([[(x + 0.5) / w, (y + 0.5) / h] for y in range(h) for x in range(w)])
    return np.concatenate([grid, np.random.default_rng(seed).uniform(-0.5, 1.5, (64, 2))])


def _escapes(objs, tri_v, o, d, scale=1.0):
    """fp64, with a margin: the ray meets no sphere and no triangle (only to choose rays; the reference decides what they hit)"""
    c, r = np.array([q["center"] for q in objs]), np.array([q["radius"] for q in objs])
    L = c - o
    tca = L @ d
    thc2 = (r + 0.01 * np.minimum(r, 100.0 * scale)) ** 2 - ((L * L).sum(axis=1) - tca * tca)
    if ((thc2 >= 0.0) & (tca + np.sqrt(np.maximum(thc2, 0.0)) > 0.0)).any():
        return False
    if tri_v is None:
        return True
    with np.errstate(all="ignore"):
        v0, e1, e2 = tri_v[:, 0], tri_v[:, 1] - tri_v[:, 0], tri_v[:, 2] - tri_v[:, 0]
        h = np.cross(d, e2)
        f = 1.0 / (e1 * h).sum(axis=1)
        sv = o - v0
        u = f * (sv * h).sum(axis=1)
        q = np.cross(sv, e1)
        v = f * (q @ d)
        t = f * (e2 * q).sum(axis=1)
        return not ((u > -0.01) & (v > -0.01) & (u + v < 1.01) & (t > 0.0)).any()


def opening_uv(sc, scale=1.0, offset=(0.0, 0.0, 0.0), n=96, seed=20261006):
    """(u, v) of n rays of the scene's camera that leave class_scene's room through its missing back wall: towards points 1000
    behind it, the first n of the seed's sequence whose ray meets nothing (_escapes).  An open_back room lets a ray escape only
    within 3.6 degrees of its axis (the floor and ceiling spheres of radius 1e4 curve away by s^2 / 2e4 at distance s: a slope beyond
    sqrt(4 * 20 / 2e4) = 0.063 meets them), and the sheet of triangles and the packed spheres stand in the way: 2 of the 448 rays of
    uv_set escape from the class's own camera and none from most others.  These points are what makes a tenth of an open scene's uv
    rays miss under every variant.  get_camera_ray's direction is pos - (llc + H u + V v): solve
    pos - llc = H u + V v + lambda (target - pos)."""
    rng = np.random.default_rng(seed)
    pos, H, V, llc = util.camera_arrays(sc.camera)
    objs, meshes = util.scene_parts(sc)
    tri_v = _tri_vertices(meshes)
    out = []
    for _ in range(100 * n):
        target = np.array([rng.uniform(-30, 30), rng.uniform(-18, 18), -1000.0]) * scale + np.asarray(offset)
        u, v, lam = np.linalg.solve(np.stack([H, V, target - pos], axis=1), pos - llc)
        if lam > 0.0 and _escapes(objs, tri_v, pos, _unit(target - pos), scale):
            out.append([u, v])
            if len(out) == n:
                break
    return np.array(out).reshape(-1, 2)


def variant_rays(name, variant):
    """-> dict(scene: Q.SCENES[name] under `variant` (None: as it is; the caller frees it), uv [448, 2] for the scene's camera (uv_set;
    an OPEN_BACK scene: and opening_uv, [544, 2]), rays [512, 6], scale).  The world rays are Q.ray_set of the scene: under a camera variant the geometry and so the set stay, under a
    placement the set of the class's own place is carried by the placement's map (origins scaled and moved, directions kept) --
    ray_set itself holds absolute lengths (a spread of at least 4, a clearance of 0.25, radius 1000 as `wall-sized`), so only the
    mapped set meets the same geometry at every scale, which is what tests/test_query_edges_cpu.py asks of tiny and huge."""
    base = Q.SCENES[name][1]()
    rays = Q.ray_set(base, N_WORLD)
    sc, s, off = base, 1.0, np.zeros(3)
    if variant is not None:
        sc = util.view_variant(base, variant)
        base.free()
        s, off = util.SCALES.get(variant, 1.0), np.array(util.FAR_OFFSET) if variant == "far" else off
    if variant in util.PLACEMENTS:
        rays = rays.copy()
        rays[:, :3] = rays[:, :3] * s + off
    uv = uv_set()
    if name in OPEN_BACK:
        uv = np.concatenate([uv, opening_uv(sc, s, off)])
    return dict(scene=sc, uv=uv, rays=rays, scale=s)


# ---- (b), (c) origins around near_R ------------------------------------------------------------------------------------------------
def shell_rays(sc, origin_radius, seed=20261002, radii=None):
    """512 rays from origins R_k u (u uniform on the sphere, R_k = ladder(near_R_of(sc, origin_radius))[k % 26], so at least 19 rays
    a radius) towards points on primitives.  -> rays [512, 6], k [512] (which rung)"""
    rng = np.random.default_rng(seed)
    radii = ladder(near_R_of(sc, origin_radius)) if radii is None else np.asarray(radii, dtype=np.float64)
    k = np.arange(N_SHELL) % len(radii)
    origins = _unit(rng.normal(size=(N_SHELL, 3))) * radii[k][:, None]
    return np.concatenate([origins, _unit(_targets(sc, rng, N_SHELL) - origins)], axis=1), k


def fixed_shell(sc, seed=20261003):
    """512 rays whose origins all lie R0 = near_R_of(sc, reach) from the world origin (to rounding): the set hint_ladder moves the
    thresholds around.  -> rays, R0"""
    R0 = near_R_of(sc, reach_of(sc))
    return shell_rays(sc, 0.0, seed, radii=[R0])[0], R0


def hint_ladder(sc, rays):
    """for rays with every |o| = R0: the origin_radius values that put near_R at R0 (1 + j 2^-m) and at R0 itself (the threshold
    of every form but one), and at those values / sqrt(0.9999) (the sign-test form's threshold then lies there); 26 hints"""
    R0 = float(np.median(np.sqrt((rays[:, :3] ** 2).sum(axis=1))))
    reach = reach_of(sc)
    rel = [0.0] + [j * 2.0 ** -m for m in LADDER_M for j in (1.0, -1.0)]
    hints = [((R0 * (1.0 + x) / f) - 1.0) / 1.5 - reach for f in (1.0, SIGN_TEST_FACTOR) for x in rel]
    assert min(hints) >= 0.0
    return hints


# ---- (d) grazing rays ----------------------------------------------------------------------------------------------------------------
def neighbour_pairs(tri_v):
    """pairs (i, j), i < j, of triangles that share an edge (two vertices equal in every coordinate).  The sheets of class_scene are
    independent random triangles and share none; the neighbours here are the exact duplicates of lopsided_mesh_scene and
    mesh_soup_scene, which share all three."""
    edges = {}
    for t, tri in enumerate(tri_v):
        keys = [tuple(v) for v in tri]
        for a, b in ((0, 1), (1, 2), (2, 0)):
            if keys[a] != keys[b]:
                edges.setdefault(frozenset((keys[a], keys[b])), []).append(t)
    return sorted({(ts[0], t) for ts in edges.values() for t in ts[1:] if t != ts[0]})


def _pick_triangles(tri_v, n):
    """up to n triangle indices: those with a neighbour first (at most half, both of a pair), the rest spread over the mesh"""
    paired = []
    for i, j in neighbour_pairs(tri_v):
        paired += [t for t in (i, j) if t not in paired]
    chosen = paired[:n // 2]
    for t in np.linspace(0, len(tri_v) - 1, min(n, len(tri_v))).astype(int):
        if len(chosen) < min(n, len(tri_v)) and int(t) not in chosen:
            chosen.append(int(t))
    return sorted(chosen)


def grazing_rays(sc, seed=20261004):
    """-> rays [n, 6] and info, a dict of arrays [n]: kind (0 sphere silhouette, 1 triangle vertex, 2 edge point, 3 edge point
    moved across the edge), target (sphere index / global triangle index), delta (the relative offset: of the radius, of the edge
    length).

    Sphere silhouettes: for up to 32 spheres of ordinary size and 4 free origins each, the ray tangent to the concentric sphere of
    radius r (1 + delta): aimed at c + r (1 + delta) n with n the unit vector perpendicular to the RAY in a random plane through
    c - o (the point of the ray nearest the centre; a point perpendicular to c - o would lie inside the silhouette by r^2 / |c - o|).
    Triangles: up to GRAZE_TRIS of each mesh, from one free origin off the triangle's plane: every vertex, three points on every
    edge, and those points moved in the plane across the edge by +-2^-k of its length."""
    rng = np.random.default_rng(seed)
    objs, meshes = util.scene_parts(sc)
    anchors = _anchors(sc, rng)
    rays, kind, target, delta = [], [], [], []
    small = [(i, o) for i, o in enumerate(objs) if o["radius"] < 1000]
    small_objs = [o for _, o in small]
    for i, o in [small[k] for k in np.linspace(0, len(small) - 1, min(GRAZE_SPHERES, len(small))).astype(int)]:
        c, r = np.array(o["center"]), o["radius"]
        for a in range(GRAZE_ORIGINS):
            org = anchors[(i + 5 * a) % 16] + rng.uniform(-0.2, 0.2, 3)
            w = c - org
            dist = float(np.linalg.norm(w))
            if dist < 1.5 * r:
                continue
            n0 = _unit(np.cross(w, rng.normal(size=3)))
            for dl in GRAZE_DELTAS:
                s = r * (1.0 + dl) / dist                  # sin of the angle between c - o and the tangent
                rays.append(np.concatenate([org, _unit(np.sqrt(1.0 - s * s) * w / dist + s * n0)]))
                kind.append(0), target.append(i), delta.append(dl)
    first = 0
    for m in meshes:
        tri_v = m["vertices"][:, :3].reshape(-1, 3, 3)
        for t in _pick_triangles(tri_v, GRAZE_TRIS):
            v = tri_v[t]
            nrm = np.cross(v[1] - v[0], v[2] - v[0])
            if not np.linalg.norm(nrm) > 1e-12:
                continue                                   # a degenerate triangle has no plane to move in
            nrm = _unit(nrm)
            size = max(np.linalg.norm(v[1] - v[0]), np.linalg.norm(v[2] - v[0]))
            for a in range(16):   # an origin at least a quarter of the triangle's size off its plane that sees its centroid
                org = anchors[(t + a) % 16] + rng.uniform(-0.2, 0.2, 3)
                if abs(np.dot(org - v[0], nrm)) > 0.25 * min(size, 4.0) and not _blocked(small_objs, org, v.mean(axis=0)):
                    break
            pts = [(1, v[k], 0.0) for k in range(3)]
            for a, b, c in ((0, 1, 2), (1, 2, 0), (2, 0, 1)):
                e = v[b] - v[a]
                out = _unit(np.cross(e, nrm))
                out = out if np.dot(out, v[c] - v[a]) < 0 else -out      # in the plane, away from the third vertex
                for f in (0.25, 0.5, 0.75):
                    p = v[a] + f * e
                    pts.append((2, p, 0.0))
                    pts += [(3, p + s * 2.0 ** -k * np.linalg.norm(e) * out, s * 2.0 ** -k) for k in GRAZE_SHIFTS for s in (1.0, -1.0)]
            for kd, p, dl in pts:
                rays.append(np.concatenate([org, _unit(p - org)]))
                kind.append(kd), target.append(first + t), delta.append(dl)
        first += len(tri_v)
    return np.array(rays), dict(kind=np.array(kind), target=np.array(target), delta=np.array(delta))


# ---- (e) axis-parallel rays ------------------------------------------------------------------------------------------------------------
def axis_directions():
    """the six axis directions with their zeros as 0.0 and as -0.0, then (+-0.6, +-0.8, 0) in its three axis placements (the zero
    alternately 0.0 and -0.0): 24 directions, each with |d|^2 = 1 to an ulp"""
    dirs = []
    for a in range(3):
        for s in (1.0, -1.0):
            for z in (0.0, -0.0):
                d = np.full(3, z)
                d[a] = s
                dirs.append(d)
    k = 0
    for a in range(3):
        for s1 in (0.6, -0.6):
            for s2 in (0.8, -0.8):
                d = np.zeros(3)
                d[a], d[(a + 1) % 3], d[(a + 2) % 3] = s1, s2, (0.0, -0.0)[k % 2]
                dirs.append(d)
                k += 1
    return np.array(dirs)


def axis_direction_index(axis, negative, minus_zero):
    """where axis_directions() holds the direction along `axis` (0 x, 1 y, 2 z) with that sign, its two zeros written as -0.0 or 0.0"""
    k = 4 * axis + 2 * int(negative) + int(minus_zero)
    d = axis_directions()[k]
    assert d[axis] == (-1.0 if negative else 1.0) and (np.signbit(np.delete(d, axis)) == bool(minus_zero)).all() and (np.delete(d, axis) == 0.0).all()
    return k


def _f32(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


def axis_rays(sc, near_R=None, scale=1.0):
    """-> rays [n, 6] and info, a dict of arrays [n]: kind (0 through a vertex, fp64 coordinates; 1 the same rounded to fp32; 2 a
    face ladder; 3 sphere centres and centre +- radius), face (ladders: 2 axis + side, else -1), step (ladders: fp32 steps outward
    from the extreme vertex coordinate, negative inside), t_point (ladder steps <= 0: the distance along the ray to the point of the
    extreme triangle the ray passes through).

    Every origin lies one diagonal of the primitives' bounding box back from the point the ray is built through, so that point
    and what surrounds it lie ahead.  A face ladder belongs to one face of the vertices' bounding box: rays parallel to the face
    whose coordinate across it takes CONSECUTIVE fp32 values from AXIS_INWARD steps inside the extreme vertex coordinate outward
    over twice the hierarchy's widening 4 * 2^-24 (near_R + |b|) (pt_intersect.h, bvh_traverse), at most AXIS_STEPS_MAX steps.  The
    fp32 boxes are internal; one of these consecutive values IS the widened plane, whatever its rounding.  Steps inside pass through
    the extreme triangle (along the line from the extreme vertex to the triangle's centroid), steps outside pass beside the vertex.
    Where there is a choice the directions are taken from which no sphere of ordinary size hides the point.
    near_R: the launch's (None: near_R_of(sc, 0)); scale: of a scaled scene (util.SCALES), for what counts as wall-sized."""
    objs, meshes = util.scene_parts(sc)
    small, tri_v = _small(objs, scale), _tri_vertices(meshes)
    near_R = near_R_of(sc, 0.0) if near_R is None else near_R
    dirs = axis_directions()
    lo = np.min([np.array(o["center"]) - o["radius"] for o in small] + ([tri_v.reshape(-1, 3).min(axis=0)] if meshes else []), axis=0)
    hi = np.max([np.array(o["center"]) + o["radius"] for o in small] + ([tri_v.reshape(-1, 3).max(axis=0)] if meshes else []), axis=0)
    back = float(np.linalg.norm(hi - lo))
    rays, kind, face, step, t_point = [], [], [], [], []

    def add(p, d, kd, fc=-1, st=0, tp=np.nan):
        # (p - back d rounds along d only where d has a non-zero component: the transverse coordinates stay exactly p's)
        rays.append(np.concatenate([np.where(d == 0.0, p, p - back * d), d]))
        kind.append(kd), face.append(fc), step.append(st), t_point.append(tp)

    def visible_first(p, candidates):
        return sorted(candidates, key=lambda k: _blocked(small, p - back * dirs[k], p))     # (stable: the given order otherwise)
    if meshes:
        verts = tri_v.reshape(-1, 3)
        for n, k in enumerate(np.linspace(0, len(verts) - 1, min(AXIS_VERTICES, len(verts))).astype(int)):
            for j in visible_first(verts[k], [(7 * n + i) % len(dirs) for i in range(len(dirs))])[:AXIS_DIRS]:
                add(verts[k], dirs[j], 0)
                add(_f32(verts[k]), dirs[j], 1)
        for a in range(3):
            for side in (0, 1):
                col = verts[:, a]
                k = int(col.argmax() if side else col.argmin())
                v, cen = verts[k], tri_v[k // 3].mean(axis=0)
                widen = 4.0 * E24 * (near_R + abs(v[a]))
                x0 = np.float32(v[a])
                ulp = float(np.spacing(np.abs(x0)))
                steps = min(int(np.ceil(2.0 * widen / ulp)) + 2, AXIS_STEPS_MAX)
                others = [b for b in range(3) if b != a]
                # two of the eight axis directions along the face (one where the ladder has more than 64 steps), signs and zero signs varying
                # (candidates: both axes of the face, both signs, the zeros -0.0 on every other one; which comes first varies by face)
                cand = [axis_direction_index(others[(side + j) % 2], (a + j + j // 2) % 2, (a + side + j) % 2) for j in range(4)]
                use = [dirs[j] for j in visible_first(v, cand)[:2 if steps <= 64 else 1]]
                assert all(d[a] == 0.0 for d in use)      # along the face: the coordinate across it is the ladder's alone
                x = x0
                for _ in range(AXIS_INWARD):
                    x = np.nextafter(x, np.float32(-np.inf if side else np.inf))
                for st in range(-AXIS_INWARD, steps + 1):
                    p = v.copy()
                    inside = (v[a] - float(x)) / (v[a] - cen[a])          # > 0: towards the centroid
                    if inside > 0.0:
                        p = v + inside * (cen - v)
                    p[a] = float(x)
                    for d in use:
                        add(p, d, 2, 2 * a + side, st, back if 0.0 < inside <= 0.9 else np.nan)
                    x = np.nextafter(x, np.float32(np.inf if side else -np.inf))
    else:
        for n, o in enumerate(small[:AXIS_VERTICES]):
            c, r = np.array(o["center"]), o["radius"]
            for j in range(4):
                d = dirs[(4 * n + j) % len(dirs)]
                t1 = np.eye(3)[int(np.argmax(d == 0.0))]          # along a zero component: across the ray, whatever d
                for off in (0.0, 1.0, -1.0):
                    add(c + off * r * t1, d, 3)
    return np.array(rays), dict(kind=np.array(kind), face=np.array(face), step=np.array(step), t_point=np.array(t_point))


def axis_set(sc, scale=1.0):
    """-> rays, info, hint: axis_rays with its ladders sized for the launch that has every origin inside near_R -- origin_radius =
    hint, the farthest origin (beyond near_R a ray keeps every box and every primitive: far_origin).  The origins do not depend on
    the ladders' lengths but for the steps themselves, which lie closer to the scene than the rays through its vertices."""
    first, _ = axis_rays(sc, None, scale)
    hint = float(np.sqrt((first[:, :3] ** 2).sum(axis=1)).max()) * (1.0 + 2.0 ** -20)
    rays, info = axis_rays(sc, near_R_of(sc, hint), scale)
    assert float(np.sqrt((rays[:, :3] ** 2).sum(axis=1)).max()) <= hint
    return rays, info, hint

"""Sphere and ray sets for the fp16 matrix form of the phase-1 filter (pt_device.h: pt_mfma16_row; pt_filter.h: filter_mfma16), shared
by the CPU emulation (tests/test_mfma16_table_cpu.py) and the GPU self-test (tests/test_gpu_mfma16_selftest.py), and the bound's
figures A, W16, ET, EL, E16 as the comment above pt_mfma16_row states them.

A SET is one rt_hip_selftest_intersect(kind 2) call: a near_R and a whole number of BLOCKS of 64 spheres and 64 rays; spheres 0..31
of a block are the matrix rows, 32..63 follow in the packed loop.  A sphere LAYOUT gives three blocks, one per ray template:
  template 0   lanes 0..31 hit sphere k through half its radius (a wall-sized radius: through 0.999 of it, from the origin's side, so
               that the ray starts within near_R); lanes 32..63 miss sphere k beyond the bound (must be dropped, see must_drop_d2);
  template 1   lanes 0..31 graze sphere k inside it (d2 = r^2 (1 - 1e-6)); 32..47 miss k = 0..15 INSIDE the bound (d2 = r^2 + W16 / 2,
               either answer is right); 48..55 start inside k = 16..23 with tca = 0 to rounding; 56..59 NaN direction; 60..63 start
               beyond near_R;
  template 2   lanes 0..31 pass through the centre of sphere k along an axis, the other two components of the direction taken from
               0.0, -0.0 and +-2^-20; 32..39 start ON sphere k's surface pointing inward, 40..47 on it pointing outward, 48..55
               outside it pointing away (tca < 0); 56..59 graze k from |o| = near_R (1 - 2^-20) (the filter's far-origin shell: such a
               ray keeps everything), 60..63 graze it from |o| = 0.999 near_R (the largest |o'|^2 the fp16 split is given to filter).
A sphere whose radius is below any rounding (the `zeros` set's radius 1e-100) gets, in lane k of every template, the pure axis ray
through its dyadic centre instead: L = s d exactly, d2 = 0 exactly, the only kind of ray that hits it.

Every fitting block is checked here, in fp64: each row sphere is exactly hit by a ray of its block and missed by more than
W16 + E16 (+ the split's residual) by another -- a sphere in the wrong row of the A operand would lose its hit or keep its miss.

The sets: limit (near_R = 250), over (the same at nextafter(250, inf): nothing fits), small (the limit layout scaled to near_R 8, 1,
2^-6), zeros (signed zeros, the origin, 2^-15 and 2^-20, concentric and identical spheres, radius ~ 0; near_R 160 and 1), kq (|kq|
near 60000: fitting spheres and their just-unfitting twins), mixed_fit (fitting, one row unfitting, fitting)."""
import numpy as np

E = 2.0 ** -24
EPSILON = 1e-8          # raytracer.h: intersect_sphere accepts t > EPSILON
NEAR_R_MAX = 250.0      # PT_MFMA16_NEAR_R_MAX
TINY_RADIUS = 1e-100    # the smallest radius rt_hip_selftest_intersect (and rt_hip_scene_create) takes


def filt_shift(max_center, near_R):
    """the self-test's launch (rt_hip_selftest_intersect): 12 e (max |c| + near_R), as a render launch forms it"""
    return 12.0 * E * (max_center + near_R) * (1.0 + 1e-9)


def center_norm(cen):
    """|c| as scene_sphere_entry rounds it up"""
    cen = np.asarray(cen, dtype=np.float64)
    return np.sqrt(cen[:, 0] * cen[:, 0] + cen[:, 1] * cen[:, 1] + cen[:, 2] * cen[:, 2]) * (1.0 + 1e-12)


def bounds(cen, rad, near_R, tol):
    """per sphere: A, W16, ET, EL, E16, |kq| and the split's residual, as pt_mfma16_row computes and its comment derives them"""
    cn = center_norm(cen)
    rad = np.asarray(rad, dtype=np.float64)
    A = (cn + near_R + tol) * (1.0 + 1e-6)
    g = np.abs(cn * cn - rad * rad)
    W16 = (A * A / 65536.0 + g / 262144.0 + A / 131072.0) * (1.0 + 1e-6)
    kq = np.abs(cn * cn - rad * rad - W16)
    ET = 3 * 2.0 ** -19 * A + 2.0 ** -20
    EL = 1.82 * 2.0 ** -19 * A * A + 1.16 * 2.0 ** -19 * kq + 6 * E * A
    E16 = 8 * 2.0 ** -19 * A * A + 1.5 * 2.0 ** -19 * kq + 2.0 ** -18 * A
    # kq is lowered by 2^-21 |kq| + 2^-23 before its split, whose own residual is at most 2^-22 |kq| + 2^-25: r2_hi16 exceeds r^2 + W16 by at most
    resid = kq * 2.0 ** -20 + 2.0 ** -22
    return dict(A=A, W16=W16, ET=ET, EL=EL, E16=E16, kq=kq, resid=resid)


def fits(cen, rad, near_R, tol):
    """the fit rule of pt_mfma16_row, restated (the CPU test sets it against the row harness)"""
    cen, rad = np.asarray(cen, dtype=np.float64), np.asarray(rad, dtype=np.float64)
    cn = center_norm(cen)
    B = bounds(cen, rad, near_R, tol)
    kq = cn * cn - (rad * rad + B["W16"])
    kq = kq - (np.abs(kq) / 2097152.0 + 1.0 / 8388608.0)
    return ((near_R <= NEAR_R_MAX) & (0.0 <= tol <= 1.0) & (cn <= 8192.0) & (rad * rad < 1e6) & (np.abs(cen) <= 4096.0).all(axis=1) &
            (np.abs(kq) <= 60000.0))


def must_drop_holds(B):
    """q''16 <= r2_hi16 - d2 + E16 and r2_hi16 <= r^2 + W16 + resid: d2 = r^2 + 2.5 W16 is dropped for certain where
    E16 < 1.5 W16 - resid"""
    return B["E16"] < 1.5 * B["W16"] - B["resid"]


def must_drop_d2(rad, B):
    """where a set's must-drop misses stand: at r^2 + 2.5 W16 if the inequality above holds for every sphere given, else at
    r^2 + W16 + resid + 1.25 E16, from E16's own formula (the residual is part of r2_hi16 by construction -- pt_mfma16_row takes it
    off kq beforehand -- so no placement inside it can be asked to drop)"""
    rad = np.asarray(rad, dtype=np.float64)
    if must_drop_holds(B).all():
        return rad * rad + 2.5 * B["W16"], True
    return rad * rad + B["W16"] + B["resid"] + 1.25 * B["E16"], False


# ---- layouts -------------------------------------------------------------------------------------------------------------------
def _unit(rng):
    v = rng.normal(size=3)
    return v / np.linalg.norm(v)


def limit_layout(scale=1.0):
    """rows: |c| from 0 to 160 in even steps, every direction, radii 0.5 .. 2; behind them 32 spheres of radius 0.75 within 160"""
    rng = np.random.default_rng(7)
    cen, rad = [], []
    for k in range(32):
        cen.append(_unit(rng) * (160.0 * k / 31.0))
        rad.append(0.5 + 1.5 * ((7 * k) % 32) / 31.0)
    for k in range(32):
        cen.append(_unit(rng) * rng.uniform(0.0, 160.0))
        rad.append(0.75)
    return np.array(cen) * scale, np.array(rad) * scale


def zeros_layout(u):
    """u = the length unit (1 at near_R 160, 2^-7 at near_R 1); 2^-15 and 2^-20 are absolute"""
    rng = np.random.default_rng(8)
    a, b = 2.0 ** -15, 2.0 ** -20
    rows = [((0.0, 0.0, 0.0), 1.0 * u), ((0.0, 0.0, 0.0), 2.0 * u),                       # at the origin, and concentric with it
            ((8 * u, 0.0, -0.0), u), ((-0.0, 8 * u, 0.0), u), ((0.0, -0.0, -8 * u), u),     # on the axes, signed zeros
            ((a, 4 * u, 0.0), u), ((4 * u, b, -0.0), u), ((b, a, 4 * u), u), ((-a, -b, -4 * u), 0.5 * u),
            ((10 * u, -6 * u, 3 * u), 1.5 * u), ((10 * u, -6 * u, 3 * u), 1.5 * u),         # identical
            ((16 * u, 0.0, 0.0), TINY_RADIUS),                                              # radius ~ 0 (r^2 = 1e-200), dyadic centre
            ((-12 * u, 5 * u, 7 * u), u), ((-12 * u, 5 * u, 7 * u), 0.5 * u),               # concentric away from the origin
            ((0.0, 0.0, 24 * u), 2 * u), ((0.0, -24 * u, 0.0), 2 * u), ((-24 * u, -0.0, 0.0), 2 * u), ((a, a, a), u), ((b, b, b), u)]
    while len(rows) < 32:
        rows.append((tuple(_unit(rng) * rng.uniform(2.0, 40.0) * u), float(rng.uniform(0.5, 2.0)) * u))
    for k in range(32):
        rows.append((tuple(_unit(rng) * rng.uniform(0.0, 40.0) * u), 0.75 * u))
    return np.array([r[0] for r in rows]), np.array([r[1] for r in rows])


# radius 0 itself: pt_mfma16_row takes it (r^2 >= 0), the shim's entry points do not (|radius| >= 1e-100): the row harness alone sees it
ZERO_RADIUS_SPHERES = [(16.0, 0.0, 0.0, 0.0), (0.0, 0.0, 0.0, 0.0), (0.125, -0.0, 2.0 ** -20, 0.0)]

# |kq| near fp16's range at near_R = 250.  A radius of 999 fits where |c|^2 - 999^2 - W16 >= -60000: |c| >= 968.6, and |c| = 970 gives
# A = 1220, W16 = 22.9, kq = -57124 (every origin within near_R is then inside the sphere: the exact test accepts it whenever tca >= 0)
KQ_FIT = [((3.0, 4.0, 5.0), 240.0), ((244.9, 0.0, 0.0), 0.5), ((141.0, 141.0, 141.0), 2.0), ((970.0, 0.0, 0.0), 999.0)]
# their twins: 245^2 = 60025 at |c|^2 = 3; |c|^2 = 60516; the wall threshold itself
KQ_UNFIT = [((1.0, 1.0, 1.0), 245.0), ((246.0, 0.0, 0.0), 0.5), ((3.0, 4.0, 5.0), 1000.0)]


def _with_rows(layout, rows, at):
    cen, rad = layout[0].copy(), layout[1].copy()
    for k, (c, r) in zip(at, rows):
        cen[k], rad[k] = c, r
    return cen, rad


# ---- rays ------------------------------------------------------------------------------------------------------------------------
def _norm(v):
    return v / np.linalg.norm(v)


def _pow2_below(x):
    return 2.0 ** np.floor(np.log2(x))


_AXIS_OTHERS = [(0.0, 0.0), (-0.0, 0.0), (0.0, -0.0), (2.0 ** -20, 0.0), (0.0, -2.0 ** -20), (-0.0, 2.0 ** -20), (-2.0 ** -20, -0.0), (-0.0, -0.0)]


def _axis_ray(k, c, near_R, pure, wide):
    a, sgn, s = k % 3, (1.0 if (k // 3) % 2 == 0 else -1.0), _pow2_below(0.04 * near_R)
    if wide:   # a wall-sized radius: along the centre's largest component, from about the origin
        a = int(np.argmax(np.abs(c)))
        sgn, s = (1.0 if c[a] >= 0 else -1.0), max(1.0, float(np.round(np.linalg.norm(c))))
    x1, x2 = (0.0, -0.0) if pure else _AXIS_OTHERS[k % 8]
    d = np.zeros(3)
    d[a], d[(a + 1) % 3], d[(a + 2) % 3] = sgn, x1, x2       # |d|^2 <= 1 + 2^-40: inside the filter's |d| <= 1.0001
    return c - s * d, d


def _graze_from(o, c, b, rng):
    """a unit direction from o that passes c at distance b"""
    L = c - o
    D = np.linalg.norm(L)
    u = L / D
    p = _norm(np.cross(u, rng.normal(size=3)))
    sin_t = b / D
    return np.sqrt(1.0 - sin_t * sin_t) * u + sin_t * p


def block_rays(template, cen, rad, B, near_R, drop_d2, seed):
    """the 64 rays of one block, their kinds and the sphere each is aimed at"""
    rays, kind, target = np.zeros((64, 6)), [None] * 64, [0] * 64
    s = 0.04 * near_R

    def make(i, k, what):
        rng = np.random.default_rng(100000 * seed + 100 * template + i)
        c, r = cen[k], rad[k]
        cn = np.linalg.norm(c)
        wide = r > 0.4 * near_R
        if wide and cn > 0:          # from the origin's side, so that the ray starts within near_R
            p = -c / cn
            d = _norm(np.cross(p, rng.normal(size=3)))
        else:
            d = _unit(rng)
            if cn + s > 0.9 * near_R:   # a centre near the rim: the ray runs outward through it, so that it starts inside near_R
                d = _norm(c / cn + 0.3 * d)
            p = _norm(np.cross(d, rng.normal(size=3)))
        if i < 32 and r < 1e-9 * near_R:
            what = "axis"
        if what == "axis":
            o, d = _axis_ray(k, c, near_R, r < 1e-9 * near_R, wide)
        elif what in ("hit", "nan"):
            o = c - s * d + (0.999 if wide else 0.5) * r * p
            if what == "nan":
                d = np.array([np.nan, d[1], d[2]]) * (-1.0 if i % 2 else 1.0)
        elif what == "miss":
            o = c - s * d + np.sqrt(drop_d2[k]) * p
        elif what == "graze":
            o = c - s * d + r * np.sqrt(1.0 - 1e-6) * p
        elif what == "margin":
            o = c - s * d + np.sqrt(r * r + 0.5 * B["W16"][k]) * p
        elif what == "inside":
            o = c + 0.3 * r * p
        elif what == "far":
            o = c - (1.3 * near_R + cn) * d
        elif what == "surf_in":
            o, d = c + r * p, _norm(-p + 0.5 * d)
        elif what == "surf_out":
            o, d = c + r * p, _norm(p + 0.5 * d)
        elif what == "away":
            o, d = c + (r + s) * p, _norm(p + 0.3 * d)
        else:   # edge, rim: from the far side of the origin, grazing inside the sphere
            o = (-c / cn if cn > 0 else _unit(rng)) * near_R * ((1.0 - 2.0 ** -20) if what == "edge" else 0.999)
            d = _graze_from(o, c, r * np.sqrt(1.0 - 1e-6), rng)
        rays[i, :3], rays[i, 3:] = o, d
        kind[i], target[i] = what, k

    for i in range(64):
        if template == 0:
            k, what = i % 32, ("hit" if i < 32 else "miss")
        elif template == 1:
            k, what = (i % 32, "graze") if i < 32 else (i - 32, "margin") if i < 48 else (i - 32, "inside") if i < 56 else \
                      (i - 56, "nan") if i < 60 else (i - 60 + 8, "far")
        else:
            k, what = (i, "axis") if i < 32 else (i - 32, "surf_in") if i < 40 else (i - 32, "surf_out") if i < 48 else \
                      (i - 32, "away") if i < 56 else (i - 56 + 4, "edge") if i < 60 else (i - 60 + 12, "rim")
        make(i, k, what)
    # a row sphere that no ray of the block misses beyond the bound (one that encloses most of the near_R ball: the kq set's radius
    # of 999) gets an aimed miss in place of a margin ray (template 1) or a ray pointing away (template 2)
    spare = list(range(32, 48)) if template == 1 else list(range(48, 56)) if template == 2 else []
    _, d2, _ = exact_tables(rays, cen, rad)
    finite = np.isfinite(rays).all(axis=1)
    beyond = ((d2[:, :32] > (rad[:32] ** 2 + B["W16"][:32] + B["E16"][:32] + B["resid"][:32])[None]) & finite[:, None]).any(axis=0)
    for j in np.nonzero(~beyond)[0]:
        make(spare.pop(0), int(j), "miss")
    return rays, np.array(kind), np.array(target)


def exact_tables(rays, cen, rad):
    """fp64: tca, d2 and intersect_sphere's answer (raytracer.c:77-118) for every (ray, sphere) pair"""
    o, d = rays[:, None, :3], rays[:, None, 3:]
    L = cen[None] - o
    tca = (L * d).sum(-1)
    d2 = (L * L).sum(-1) - tca * tca
    r2 = (rad * rad)[None]
    with np.errstate(invalid="ignore"):
        thc = np.sqrt(np.maximum(r2 - d2, 0.0))
        t0, t1 = tca - thc, tca + thc
        t = np.where(t0 < 0, t1, t0)
        hit = (tca >= 0) & (d2 <= r2) & (t > EPSILON)
    return tca, d2, hit


# ---- sets ------------------------------------------------------------------------------------------------------------------------
def _make_set(name, near_R, layouts, seed):
    """layouts: (cen, rad, templates, fits) -- one block per template"""
    max_center = max(float(center_norm(cen).max()) for cen, _, _, _ in layouts)
    tol = filt_shift(max_center, near_R)
    blocks = []
    for cen, rad, templates, fit in layouts:
        B = bounds(cen, rad, near_R, tol)
        drop_d2, plain = must_drop_d2(rad[:32], {k: v[:32] for k, v in B.items()})
        drop_d2 = np.concatenate([drop_d2, np.zeros(32)])
        for t in templates:
            rays, kind, target = block_rays(t, cen, rad, B, near_R, drop_d2, seed)
            blocks.append(dict(cen=cen, rad=rad, fits=fit, template=t, rays=rays, kind=kind, target=target, bounds=B, drop_plain=plain))
    S = dict(name=name, near_R=near_R, tol=tol, blocks=blocks)
    _check_set(S)
    return S


def _check_set(S):
    for n, b in enumerate(S["blocks"]):
        assert (fits(b["cen"][:32], b["rad"][:32], S["near_R"], S["tol"]).all()) == b["fits"], (S["name"], n)
        if not b["fits"]:
            continue
        B = b["bounds"]
        tca, d2, hit = exact_tables(b["rays"], b["cen"], b["rad"])
        finite = np.isfinite(b["rays"]).all(axis=1)
        hit_rows = (hit & finite[:, None])[:, :32]
        assert hit_rows.any(axis=0).all(), (S["name"], n, "a row sphere is hit by no ray of its block", np.nonzero(~hit_rows.any(axis=0))[0])
        out = (d2[:, :32] > (b["rad"][:32] ** 2 + B["W16"][:32] + B["E16"][:32] + B["resid"][:32])[None]) & finite[:, None]
        assert out.any(axis=0).all(), (S["name"], n, "a row sphere is missed beyond the bound by no ray of its block")
        aimed = (b["kind"] == "miss")
        assert out[aimed, b["target"][aimed]].all()
        within = (b["rays"][:, :3] ** 2).sum(axis=1) <= S["near_R"] ** 2
        assert within[np.isin(b["kind"], ("hit", "miss", "graze", "margin", "inside", "axis", "surf_in", "surf_out", "away", "edge", "rim"))].all(), \
            (S["name"], n, "a ray meant to be filtered starts beyond near_R")
        assert not within[b["kind"] == "far"].any()


def _all_sets():
    T = (0, 1, 2)
    lim = limit_layout()
    out = [_make_set("limit", 250.0, [(*lim, T, True)], 1),
           _make_set("over", float(np.nextafter(250.0, np.inf)), [(*lim, T, False)], 1)]
    for tag, near_R in (("small-8", 8.0), ("small-1", 1.0), ("small-2^-6", 2.0 ** -6)):
        out.append(_make_set(tag, near_R, [(*limit_layout(near_R / 250.0), T, True)], 2))
    out.append(_make_set("zeros-160", 160.0, [(*zeros_layout(1.0), T, True)], 3))
    out.append(_make_set("zeros-1", 1.0, [(*zeros_layout(2.0 ** -7), T, True)], 3))
    out.append(_make_set("kq", 250.0, [(*_with_rows(lim, KQ_FIT, (0, 1, 2, 3)), T, True), (*_with_rows(lim, KQ_UNFIT, (5, 17, 31)), T, False)], 4))
    out.append(_make_set("mixed_fit", 250.0, [(*lim, (0,), True), (*_with_rows(lim, KQ_UNFIT[1:2], (17,)), (1,), False), (*lim, (2,), True)], 5))
    return out


SETS = {S["name"]: S for S in _all_sets()}


def arrays(S):
    """a set as rt_hip_selftest_intersect takes it: rays [n, 6] and prims [n, 4] (cx cy cz radius), n = 64 blocks"""
    rays = np.ascontiguousarray(np.concatenate([b["rays"] for b in S["blocks"]]))
    prims = np.ascontiguousarray(np.concatenate([np.concatenate([b["cen"], b["rad"][:, None]], axis=1) for b in S["blocks"]]))
    return rays, prims

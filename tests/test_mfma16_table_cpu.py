"""The A-operand rows of the fp16 matrix form of the phase-1 filter (pt_device.h, pt_mfma16_row), built on the host by
tests/mfma16_row_harness.cpp, and a numpy emulation of the device's side of the contraction (pt_filter.h, filter_mfma16).

  - a row's layout; hi + lo of a centre component equals the component itself where that has at most 20 significant bits
    (room corners, halves, quarters -- then it is the fp32 value exactly) and is within 2^-22 relative + 2^-25 of it
    otherwise: 24 bits do not split into two 11-bit halves in general, and that residual is part of the bound W16 covers;
    kqh + kql is at most |c|^2 - r^2 - W16 and within 2^-20 relative of it;
  - adversarial spheres: a centre on a room corner, radius 1e-3, a radius just under the wall threshold, kq near fp16's range;
  - spheres out of range are not flagged: a wall-sized radius, a far centre, kq beyond 60000, near_R beyond the form's limit, NaN;
  - the emulation on config 4's scene: every (ray, sphere) pair with tca >= 0 and d2 <= r^2 -- a superset of what the exact test
    accepts -- is kept, and the pairs the matrix form keeps although the packed-fp32 form's widening would drop them are fewer
    than 2 % of the evaluations (beyond that phase 2 would eat what phase 1 saves);
  - the shared sets of tests/mfma16_vectors.py (near_R at 250 and just past it, down to 2^-6, signed zeros and tiny components, |kq| near
    60000 and the just-unfitting twins, a block with one unfitting row): every row fits or not as the set states and as the fit rule
    restated there says, a fitting row passes the layout checks, an unfitting one is all zeros, and the emulation keeps every pair
    with tca >= 0 and d2 <= r^2 on every fitting block.  The emulation is not the device -- the device's split rounds differently --:
    this checks the vectors and the bound's arithmetic, the GPU self-test checks the kernel on the same sets."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "raytracer.c_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mfma16_vectors as V   # noqa: E402


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mfma16") / "mfma16_row_harness")
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "raytracer.c_amd", "csrc"),
                        "-o", exe, os.path.join(ROOT, "tests", "mfma16_row_harness.cpp")], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr

    def rows(spheres, near_R, tol=0.0):
        text = "".join("%s %s %s %s %s %s\n" % tuple(float(x).hex() for x in (*s, near_R, tol)) for s in spheres)
        p = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert p.returncode == 0, p.stderr
        out = []
        for line in p.stdout.splitlines():
            f = line.split()
            halves = np.array([int(h, 16) for h in f[1:17]], dtype=np.uint16).view(np.float16).astype(np.float64)
            out.append((int(f[0]), halves, float.fromhex(f[17]), float.fromhex(f[18])))
        return out
    return rows


def _check_row(s, row, near_R):
    fits, h, W16, A = row
    assert fits == 1, s
    c, r = np.array(s[:3]), s[3]
    assert h[0] == h[3] and h[1] == h[4] and h[2] == h[5]
    assert (h[9:12] == 1.0).all() and (h[14:16] == 0.0).all()
    for a in range(3):
        v = h[a] + h[6 + a]
        assert abs(v - c[a]) <= abs(c[a]) * 2.0 ** -22 + 2.0 ** -25
        if c[a] * 2.0 ** 14 == np.round(c[a] * 2.0 ** 14) and abs(c[a]) < 64:   # at most 20 bits: the split is exact
            assert v == float(np.float32(c[a])) == c[a]
    cc = float(np.dot(c, c))
    kq = h[12] + h[13]
    target = cc - r * r - W16
    assert kq <= target + 1e-9 * (1 + cc), (kq, target)
    assert target - kq <= abs(target) * 2.0 ** -20 + 2.0 ** -22 + 1e-9 * (1 + cc)
    assert W16 >= A * A / 65536.0


def test_rows_of_random_and_adversarial_spheres(harness):
    rng = np.random.default_rng(11)
    near_R = 160.0
    spheres = [(*rng.uniform(-60, 60, 3), float(10 ** rng.uniform(-3, 1.2))) for _ in range(300)]
    spheres += [(320 / 9.0, 20.0, -30.0, 2.0), (35.5, -20.0, 60.0, 1.0), (-35.5, 20.0, -30.0, 0.25),   # room corners
                (1.5, 2.25, -3.125, 1e-3), (0.0, 0.0, 0.0, 1e-3),                                      # radius 1e-3
                (3.0, 4.0, 5.0, 240.0),                                                                # the largest radius whose kq fits fp16 (|kq| <= 60000)
                (244.9, 0.0, 0.0, 0.5), (141.0, 141.0, 141.0, 2.0)]                                    # kq near fp16's range
    for s, row in zip(spheres, harness(spheres, near_R)):
        _check_row(s, row, near_R)


def test_spheres_out_of_range_are_not_flagged(harness):
    ok = (1.0, 2.0, 3.0, 1.0)
    assert harness([ok], 160.0)[0][0] == 1
    bad = [(0.0, -10020.0, 0.0, 10000.0), (1.0, 2.0, 3.0, 1000.0), (5000.0, 0.0, 0.0, 1.0), (246.0, 0.0, 0.0, 1.0),
           (3.0, 4.0, 5.0, 999.999),   # just under the wall threshold: kq = -1e6 is beyond fp16, the sphere keeps the packed loop
           (float("nan"), 0.0, 0.0, 1.0), (1.0, 2.0, 3.0, float("nan")), (1.0, float("inf"), 3.0, 1.0)]
    for s, row in zip(bad, harness(bad, 160.0)):
        assert row[0] == 0, s
    assert harness([ok], 250.5)[0][0] == 0 and harness([ok], float("inf"))[0][0] == 0


def _rtz16(x):
    """fp32 array -> fp16 rounded towards zero (v_cvt_pkrtz_f16_f32), as float64"""
    with np.errstate(over="ignore"):   # (a ray from beyond near_R: |o'|^2 past fp16's range, as on the device; such a ray keeps everything)
        h = x.astype(np.float16)
    over = np.abs(h.astype(np.float64)) > np.abs(x.astype(np.float64))
    h = np.where(over, np.nextafter(h, np.float16(0)), h)
    return h.astype(np.float64)


def _split(x, parts):
    out, rest = [], x.astype(np.float32)
    for _ in range(parts):
        p = _rtz16(rest)
        out.append(p)
        rest = (rest.astype(np.float64) - p).astype(np.float32)   # exact in fp32
    return out


def _emulate(H, o, d, tol, near_R):
    """the device's side of the contraction against the rows H [32, 16]: -> keep bits [n, 32] and the rays the filter looks at at all
    (the others start beyond near_R by filter_ray's fp32 rule and keep everything)"""
    # the device's ray (filter_ray, SHIFT): fp32, pulled back
    o32 = (o - tol * d).astype(np.float32)
    d32 = d.astype(np.float32)
    od = (o32.astype(np.float64) * d32).sum(-1).astype(np.float32)
    oo = (o32.astype(np.float64) ** 2).sum(-1).astype(np.float32)

    def contract(x, w, s):
        xs = [_split(x[:, a], 2) for a in range(3)]
        ws = _split(w, 3)
        B = np.stack([xs[0][0], xs[1][0], xs[2][0], xs[0][1], xs[1][1], xs[2][1], xs[0][0], xs[1][0], xs[2][0], ws[0], ws[1], ws[2],
                      np.full(len(w), s), np.full(len(w), s), np.zeros(len(w)), np.zeros(len(w))], axis=1)   # n x 16
        acc = np.zeros((len(w), 32), dtype=np.float32)
        for kk in range(16):                                # fp32 accumulation, one rounding per term
            acc = (acc.astype(np.float64) + B[:, kk][:, None] * H[None, :, kk]).astype(np.float32)
        return acc
    t16 = contract(d32, -od, 0.0)
    l16 = contract(-2.0 * o32, oo, 1.0)
    q16 = (t16.astype(np.float64) * np.abs(t16) - l16).astype(np.float32)
    return ~(np.signbit(q16)), oo <= np.float32(near_R * near_R * 0.9999)


def test_emulated_matrix_filter_is_conservative_and_tight_on_config4(harness):
    from rt_amd import scene as S
    sc = S.build_scene(4, 1920, 1080, 1)
    objs = [sc.objects[i] for i in range(sc.n_objects)]
    small = [(o.center.x, o.center.y, o.center.z, float(o.radius)) for o in objs if o.radius < 1000]
    assert len(small) == 32
    cen, rad = np.array([s[:3] for s in small]), np.array([s[3] for s in small])
    reach = float((np.linalg.norm(cen, axis=1) + rad).max())
    near_R = 1.5 * (50.0 + reach) + 1.0
    rows = harness(small, near_R)
    assert all(r[0] == 1 for r in rows)
    H = np.array([r[1] for r in rows])                      # 32 x 16
    e = 2.0 ** -24
    cn = np.linalg.norm(cen, axis=1)
    tol = 12 * e * (10020.0 + near_R)
    rng = np.random.default_rng(5)
    n = 6000
    half_w = 20.0 * 16 / 9
    o = rng.uniform([-half_w, -20, -30], [half_w, 20, 60], (n, 3))
    k = rng.integers(0, 32, n // 2)                        # half of the rays start ON a sphere, pointing away from it or along it
    nrm = rng.normal(size=(n // 2, 3))
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    o[: n // 2] = cen[k] + nrm * rad[k][:, None]
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    d[: n // 4] += nrm[: n // 4] * 1.0001                   # leaving the surface, many at grazing angles
    d /= np.linalg.norm(d, axis=1)[:, None]
    # the exact quantities
    L = cen[None] - o[:, None]
    tca = (L * d[:, None]).sum(-1)
    d2 = (L * L).sum(-1) - tca * tca
    may_hit = (tca >= 0) & (d2 <= rad[None] ** 2)
    keep16, _ = _emulate(H, o, d, tol, near_R)
    assert not (may_hit & ~keep16).any(), "the emulated matrix form drops a pair with tca >= 0 and d2 <= r^2"
    # the packed-fp32 form's decision, by its widening (40 e A^2 + 12 e g) in exact arithmetic
    A = cn + near_R
    W32 = (40 * e * A * A + 12 * e * np.abs(cn * cn - rad * rad))[None]
    Lp = cen[None] - (o - tol * d)[:, None]
    tp = (Lp * d[:, None]).sum(-1)
    keep32 = ~(tp * np.abs(tp) - ((Lp * Lp).sum(-1) - rad[None] ** 2 - W32) < 0)
    share = float((keep16 & ~keep32 & ~may_hit).mean())
    print("false keeps of the matrix form beyond the packed form's: %.4f %% of %d evaluations" % (100 * share, keep16.size))
    assert share < 0.02
    assert (~keep16).mean() > 0.8, "the filter should reject most pairs"


@pytest.mark.parametrize("name", list(V.SETS))
def test_rows_of_the_shared_sets_fit_as_stated(harness, name):
    S = V.SETS[name]
    for n, b in enumerate(S["blocks"]):
        spheres = [(*b["cen"][k], b["rad"][k]) for k in range(32)]
        rows = harness(spheres, S["near_R"], S["tol"])
        said = V.fits(b["cen"][:32], b["rad"][:32], S["near_R"], S["tol"])
        assert [r[0] for r in rows] == [int(f) for f in said], (name, n)
        assert all(r[0] == 1 for r in rows) == b["fits"], (name, n)
        for k, (s, row) in enumerate(zip(spheres, rows)):
            if row[0]:
                _check_row(s, row, S["near_R"])
                B = b["bounds"]
                assert row[2] == pytest.approx(B["W16"][k], rel=1e-12) and row[3] == pytest.approx(B["A"][k], rel=1e-12)
            else:
                assert (row[1] == 0.0).all() and not np.signbit(row[1]).any(), (name, n, k)
    if name == "over":
        assert not any(r[0] for r in rows)


@pytest.mark.parametrize("near_R", [160.0, 1.0])
def test_rows_of_radius_zero(harness, near_R):
    """a radius of exactly 0 fits the form (the shim's entry points ask |radius| >= 1e-100, so only the row builder ever sees it)"""
    spheres = [(x * near_R / 160.0, y, z, r) for x, y, z, r in V.ZERO_RADIUS_SPHERES]
    tol = V.filt_shift(16.0 * near_R / 160.0, near_R)
    for s, row in zip(spheres, harness(spheres, near_R, tol)):
        _check_row(s, row, near_R)


@pytest.mark.parametrize("name", list(V.SETS))
def test_emulated_matrix_filter_is_conservative_on_the_shared_sets(harness, name):
    S = V.SETS[name]
    looked_at = 0
    for n, b in enumerate(S["blocks"]):
        rows = harness([(*b["cen"][k], b["rad"][k]) for k in range(32)], S["near_R"], S["tol"])
        if not b["fits"]:
            assert not all(r[0] for r in rows)
            continue
        H = np.array([r[1] for r in rows])
        ok = np.isfinite(b["rays"]).all(axis=1)
        rays = b["rays"][ok]
        keep16, near = _emulate(H, rays[:, :3], rays[:, 3:], S["tol"], S["near_R"])
        tca, d2, hit = V.exact_tables(rays, b["cen"][:32], b["rad"][:32])
        may_hit = (tca >= 0) & (d2 <= (b["rad"][:32] ** 2)[None])
        assert not (hit & ~may_hit).any()
        lost = may_hit & ~keep16 & near[:, None]
        assert not lost.any(), (name, n, "the emulated matrix form drops a pair with tca >= 0 and d2 <= r^2", np.argwhere(lost)[:4])
        assert not near[b["kind"][ok] == "far"].any() and not near[b["kind"][ok] == "edge"].any()
        assert near[np.isin(b["kind"][ok], ("hit", "miss", "graze", "margin", "rim"))].all(), (name, n)
        looked_at += int(near.sum())
        aimed = np.nonzero(near & (b["kind"][ok] == "miss"))[0]
        kept = keep16[aimed, b["target"][ok][aimed]]
        print("%s block %d: the emulation keeps %d of %d aimed must-drop misses, drops %.1f %% of all pairs"
              % (name, n, kept.sum(), len(aimed), 100.0 * (~keep16[near]).mean()))
    assert (looked_at > 0) == any(b["fits"] for b in S["blocks"])

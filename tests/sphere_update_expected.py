"""What a scene derives from its spheres (raytracer.c_amd/csrc/scene_spheres.h), restated in numpy, the stand-alone harness that
prints the header's own results (tests/sphere_update_harness.cpp), and the sphere moves the tests of rt_hip_scene_update_spheres
share (tests/test_sphere_update_cpu.py, tests/test_gpu_sphere_update.py, tests/sphere_update_diag_child.py).

Spheres everywhere: float64 (n, 4), cx cy cz radius, in object order."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WALLS = 8


def expected(spheres):
    """-> dict(entry (n, 6), geom4 (n, 4), reach_spheres, max_center, wide_range, n_big, big_r (8), big_c (8), radii_ok): every
    operation in the header's order, unfused"""
    s = np.asarray(spheres, dtype=np.float64).reshape(-1, 4)
    n = len(s)
    c, r = s[:, :3], s[:, 3]
    entry = np.zeros((n, 6))
    with np.errstate(all="ignore"):
        entry[:, :3] = c
        entry[:, 3] = r * r
        entry[:, 4] = np.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2]) * (1.0 + 1e-12)
        ar = np.abs(r)
        reach_part = np.where(ar < 1000.0, np.fmax(0.0, entry[:, 4] + ar), 0.0)
        wide = ~(entry[:, 4] <= 1e17) | ~(ar <= 1e17)
    nb = 0
    while nb < WALLS and nb < n and ar[nb] >= 1000.0 and ar[nb] <= 1e17:
        nb += 1
    nb &= ~1
    big_r, big_c = np.zeros(WALLS), np.zeros(WALLS)
    big_r[:nb], big_c[:nb] = ar[:nb], entry[:nb, 4]
    return dict(entry=entry, geom4=entry[:, :4].copy(), reach_spheres=float(np.fmax.reduce(reach_part, initial=0.0)),
                max_center=float(np.fmax.reduce(np.fmax(0.0, entry[:, 4]), initial=0.0)), wide_range=bool(wide.any()), n_big=nb,
                big_r=big_r, big_c=big_c, radii_ok=bool(((ar >= 1e-100) & (ar <= 1e100)).all()))


def compile_harness(out_dir, extra=("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")):
    """g++ build of tests/sphere_update_harness.cpp as a stand-alone program, under AddressSanitizer and UBSan"""
    out = os.path.join(str(out_dir), "sphere_update_main")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off"] + list(extra) +
                   ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "raytracer.c_amd", "csrc"),
                    os.path.join(ROOT, "tests", "sphere_update_harness.cpp"), "-o", out], check=True)
    return out


def run_harness(prog, lists):
    """the program over `lists` of spheres -> one dict per list, in expected()'s form"""
    text = []
    for s in lists:
        s = np.ascontiguousarray(s, dtype=np.float64).reshape(-1, 4)
        text.append("%d %s" % (len(s), " ".join("%016x" % u for u in s.view(np.uint64).ravel())))
    out = subprocess.run([prog], input="\n".join(text) + "\n", capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = out.stdout.strip().splitlines()
    assert len(lines) == len(lists)
    res = []
    for s, line in zip(lists, lines):
        n, w = len(np.asarray(s).reshape(-1, 4)), line.split()
        assert len(w) == 10 * n + 2 + 2 + 16 + 1

        def f64(words):
            return np.array([int(x, 16) for x in words], dtype=np.uint64).view(np.float64)
        res.append(dict(entry=f64(w[:6 * n]).reshape(n, 6), geom4=f64(w[6 * n:10 * n]).reshape(n, 4),
                        reach_spheres=float(f64(w[10 * n:10 * n + 1])[0]), max_center=float(f64(w[10 * n + 1:10 * n + 2])[0]),
                        wide_range=bool(int(w[10 * n + 2], 16)), n_big=int(w[10 * n + 3], 16), big_r=f64(w[10 * n + 4:10 * n + 12]),
                        big_c=f64(w[10 * n + 12:10 * n + 20]), radii_ok=w[-1] == "1"))
    return res


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool((a.view(np.uint64) == b.view(np.uint64)).all())


def mismatch(got, want):
    """-> '' or what differs between two results of expected()'s form: floats by their bits"""
    for f in ("entry", "geom4", "big_r", "big_c"):
        if not same_bits(got[f], want[f]):
            return f
    for f in ("reach_spheres", "max_center"):
        if not same_bits(np.float64(got[f]), np.float64(want[f])):
            return f"{f}: {got[f]!r} != {want[f]!r}"
    for f in ("wide_range", "n_big", "radii_ok"):
        if f in got and f in want and got[f] != want[f]:
            return f"{f}: {got[f]!r} != {want[f]!r}"
    return ""


# ---- scenes and moves ----------------------------------------------------------------------------------------------------------
def spheres_of(sc):
    """the (n_objects, 4) spheres of a Scene"""
    return np.array([[o.center.x, o.center.y, o.center.z, o.radius] for o in (sc.objects[i] for i in range(sc.n_objects))],
                    dtype=np.float64).reshape(-1, 4)


def move_scene(sc, spheres):
    """writes centres and radii into the host scene's object array: the scene a fresh GpuScene, the oracle and the C host see"""
    from rt_amd import abi
    for i, (x, y, z, r) in enumerate(np.asarray(spheres, dtype=np.float64).reshape(-1, 4)):
        sc.objects[i].center = abi.Vec3(float(x), float(y), float(z))
        sc.objects[i].radius = float(r)


def jitter(s, seed=11):
    """(b): every small sphere's centre moved by up to 0.4 and its radius scaled by 0.9 .. 1.1 (config 4's packing leaves the
    spheres inside the room; they may now overlap, which the tracer does not mind)"""
    rng = np.random.default_rng(seed)
    out = np.array(s, dtype=np.float64)
    small = np.abs(out[:, 3]) < 1000.0
    out[small, :3] += rng.uniform(-0.4, 0.4, (int(small.sum()), 3))
    out[small, 3] *= rng.uniform(0.9, 1.1, int(small.sum()))
    return out


def translated(s, by=40.0):
    """(c): everything 40 along x, walls included: reach, near_R and the tables change"""
    out = np.array(s, dtype=np.float64)
    out[:, 0] += by
    return out


def wall_shrunk(s, wall=3, radius=500.0):
    """(d): leading wall `wall` keeps its surface point nearest the origin and gets radius 500: no longer wall-sized, so the
    leading walls end before it (three are left, one whole pair: n_big 6 -> 2) and the reach grows to |centre| + 500"""
    out = np.array(s, dtype=np.float64)
    c, r = out[wall, :3].copy(), out[wall, 3]
    d = np.sqrt((c * c).sum())
    out[wall, :3] = c / d * (d - r + radius)
    out[wall, 3] = radius
    return out


def far_centre(s, which=5, at=2e17):
    """(e): one sphere's centre sent to 2e17 along x: wide_range.  A WALL by default: a wall-sized sphere is no part of the reach,
    which a launch needs below 1e15"""
    out = np.array(s, dtype=np.float64)
    out[which, 0] = at
    return out


MOVES = {"identity": lambda s: np.array(s, dtype=np.float64), "jitter": jitter, "translate": translated, "wall_shrunk": wall_shrunk}

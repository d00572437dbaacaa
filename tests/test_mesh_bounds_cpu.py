"""What a scene derives from the bounds of its triangles' corners, without a device: scene_mesh_centre and scene_mesh_bounds
(raytracer.c_amd/csrc/bvh_build.h), the one text that rt_hip_scene_create and rt_hip_scene_update_vertices share, run as a
stand-alone program under AddressSanitizer and UBSan (tests/mesh_bounds_harness.cpp) and compared bit for bit with the same
formulas written in numpy fp64.  The two reductions before it (lo, hi, then r2 about the centre) are the callers' and are made
here in numpy, over the corners as the kernels see them: v0, v0 + e1, v0 + e2.

The point mesh: pi R R underflows to 0 with R = 1e-300 and the box's half area is 0, so the formula's `<=` calls it round; that is
what creation has always computed for it, and the test asks for the formula's answer."""
import os
import subprocess

import numpy as np
import pytest

import bvh_sweep_meshes as M
from conftest import ROOT

UP = np.nextafter
SLACK = np.float64(1.0 + 1e-9)
TAU = np.float64(1.1368683772161603e-13)   # 2^-43


def corners(tris):
    p = np.asarray(tris, dtype=np.float64).reshape(-1, 3, 3)
    e1, e2 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    return np.concatenate([p[:, 0], p[:, 0] + e1, p[:, 0] + e2])


def centre(lo, hi):
    return 0.5 * lo + 0.5 * hi


def reductions(tris):
    """lo, hi, r2: the callers' part"""
    with np.errstate(over="ignore", invalid="ignore"):
        c = corners(tris)
        lo, hi = c.min(axis=0), c.max(axis=0)
        d = c - centre(lo, hi)
        r2 = max(np.float64(0.0), ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).max())
    return lo, hi, np.float64(r2)


def expected(lo, hi, r2):
    with np.errstate(over="ignore", invalid="ignore"):
        c = centre(lo, hi)
        R = np.sqrt(r2) * SLACK + np.float64(1e-300)
        if not R < np.inf:
            R = np.float64(np.inf)
        c_norm = np.sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]) * np.float64(1.0 + 1e-12)
        a, b, e = hi - lo
        rnd = bool(np.float64(3.14159265358979) * R * R <= 0.5 * ((a * b + b * e) + e * a))
        tau = TAU * (c_norm + R) if R < 1e150 else np.float64(-1.0)
    return dict(c=c, R=np.float64(R), c_norm=np.float64(c_norm), tau=np.float64(tau), round=rnd)


def radius_edge():
    """s with fl(s (1 + 1e-9)) + 1e-300 == 1e150 exactly, and the double below it"""
    s = np.float64(1e150) / SLACK
    for _ in range(64):
        s = UP(s, np.float64(0.0))
    for _ in range(128):
        if s * SLACK + np.float64(1e-300) >= 1e150:
            break
        s = UP(s, np.float64(np.inf))
    return UP(s, np.float64(0.0)), s


def cases():
    n257 = np.array(M.mesh("n257")) * 3.0   # the suite's n257: the seeded shell of tests/bvh_sweep_meshes.py (no archive holds it)
    out = {"one_triangle": reductions([[[0.5, -1.0, 2.0], [3.0, 0.25, -1.5], [-2.0, 4.0, 0.75]]]),
           "point": reductions(np.full((1, 3, 3), 1.75)),
           "flat_square": reductions([[[-1, -1, 0], [1, -1, 0], [1, 1, 0]], [[-1, -1, 0], [1, 1, 0], [-1, 1, 0]]]),
           "n257_x3": reductions(n257),
           "near_1e160": reductions([[[1e160, -2e160, 0.5e160], [-1e160, 1e160, 1e160], [0.0, 3e160, -1e160]]])}
    half = np.full(3, 5e149)
    below, at = radius_edge()
    out["R_below_1e150"] = (-half, half, below * below)
    out["R_at_1e150"] = (-half, half, at * at)
    return out


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    """the sanitized program, run once over every case"""
    prog = os.path.join(str(tmp_path_factory.mktemp("mesh_bounds")), "mesh_bounds_main")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "raytracer.c_amd", "csrc"),
                    os.path.join(ROOT, "tests", "mesh_bounds_harness.cpp"), "-o", prog], check=True)
    c = cases()
    text = "\n".join(" ".join("%016x" % u for u in np.concatenate([lo, hi, [r2]]).astype(np.float64).view(np.uint64)) for lo, hi, r2 in c.values())
    out = subprocess.run([prog], input=text + "\n", capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = out.stdout.strip().splitlines()
    assert len(lines) == len(c)
    got = {}
    for name, line in zip(c, lines):
        w = line.split()
        f = np.array([int(x, 16) for x in w[:9]], dtype=np.uint64).view(np.float64)
        got[name] = dict(centre=f[0:3], c=f[3:6], R=f[6], c_norm=f[7], tau=f[8], round=w[9] == "1")
    return c, got


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64).tolist()


@pytest.mark.parametrize("name", list(cases()))
def test_header_equals_the_numpy_restatement(results, name):
    c, got = results
    g, want = got[name], expected(*c[name])
    print(name, {k: (v.tolist() if hasattr(v, "tolist") else v) for k, v in g.items()})
    assert bits(g["centre"]) == bits(want["c"]) == bits(g["c"]), f"{name}: centre {g['centre']}, {g['c']}, numpy {want['c']}"
    for f in ("R", "c_norm", "tau"):
        assert bits(g[f]) == bits(want[f]), f"{name}: {f} {g[f]!r}, numpy {want[f]!r}"
    assert g["round"] == want["round"], f"{name}: round {g['round']}, numpy {want['round']}"


def test_the_edges_fall_where_the_rules_say(results):
    c, got = results
    assert got["point"]["R"] == 1e-300 and got["point"]["c"].tolist() == [1.75] * 3 and got["point"]["tau"] > 0
    lo, hi, _ = c["flat_square"]
    assert (hi - lo).tolist() == [2.0, 2.0, 0.0] and got["flat_square"]["R"] == np.sqrt(2.0) * SLACK + 1e-300
    assert not got["flat_square"]["round"], "pi 2 > the flat box's half area of 2"
    assert 0 < got["n257_x3"]["R"] < 100 and got["n257_x3"]["tau"] == TAU * (got["n257_x3"]["c_norm"] + got["n257_x3"]["R"])
    far = got["near_1e160"]
    assert c["near_1e160"][2] == np.inf and far["R"] == np.inf and far["tau"] == -1.0 and np.isfinite(far["c"]).all()
    # the hull condition's edge: flags below 1e150, none at it
    below, at = got["R_below_1e150"], got["R_at_1e150"]
    assert at["R"] == 1e150 and below["R"] == UP(np.float64(1e150), np.float64(0.0)), (below["R"], at["R"])
    assert below["tau"] == TAU * (below["c_norm"] + below["R"]) > 0 and at["tau"] == -1.0

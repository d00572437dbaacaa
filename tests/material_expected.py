"""What a scene derives from its materials, restated in scalar Python (floats are IEEE doubles, every operation on its own:
nothing fuses), for the CPU test of raytracer.c_amd/csrc/scene_materials.h (tests/material_harness.cpp) and the GPU test of the
material update (tests/test_gpu_material_update.py); and the helpers both share: a host scene's materials in the shim's numbering
(spheres, then mesh m at n_objects + m), writing new ones into a host scene, and the comparison of records -- a NaN equals a NaN
(a black colour's 0 * inf; its sign bit is the machine's), every other word by its bits."""
import math
import os
import struct
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M_DEFAULT, M_REFLECTION, M_REFRACTION, M_CHECKERED = 2, 4, 8, 16
REFRACT, CHECKER, MIRROR_GLASS = 1, 2, 4          # the class bits (SCENE_MATERIAL_*)
LIMIT = 1e100


def material_ok(color, emission):
    """rt_hip_scene_create's rule: colour in [0, 1e100] (-0.0 is in), |emission| <= 1e100, no NaN"""
    return all(c >= 0.0 and c <= LIMIT for c in color) and all(abs(e) <= LIMIT for e in emission)


def _div(a, b):
    """a / b as IEEE does it"""
    if b == 0.0:
        if a == 0.0 or a != a:
            return math.nan
        return math.copysign(math.inf, a) * math.copysign(1.0, b)
    return a / b


def _mul(a, b):
    if (math.isinf(a) and b == 0.0) or (math.isinf(b) and a == 0.0):
        return math.nan
    return a * b


def record(flags, color, emission):
    """the 8 doubles of an object: prob by the two compares, inv = 1 / prob, colour * inv, the emission, the flags' bit pattern"""
    yz = color[1] if color[1] > color[2] else color[2]
    prob = color[0] if color[0] > yz else yz
    inv = _div(1.0, prob)
    bits = struct.unpack("<d", struct.pack("<Q", int(flags) & 0xFFFFFFFF))[0]
    return [prob, _mul(color[0], inv), _mul(color[1], inv), _mul(color[2], inv), emission[0], emission[1], emission[2], bits]


def _fmax(a, b):
    """C's fmax: a NaN gives way to the other"""
    if a != a:
        return b
    if b != b:
        return a
    return a if a > b else b


def emission_part(emission):
    return _fmax(abs(emission[0]), _fmax(abs(emission[1]), abs(emission[2])))


def class_part(flags):
    both = M_REFLECTION | M_REFRACTION
    return (REFRACT if flags & M_REFRACTION else 0) | (CHECKER if flags & M_CHECKERED else 0) | (MIRROR_GLASS if flags & both == both else 0)


def expected(materials, flags):
    """materials (n, 6: colour, emission), flags (n,) -> dict(material (n, 8), color_raw (n, 3), max_emission, classes, class_part
    (n,), emission_part (n,), ok (n,), flags (n,)); the two scalars over the objects material_ok accepts"""
    m = np.asarray(materials, dtype=np.float64).reshape(-1, 6)
    f = np.asarray(flags).reshape(-1).astype(np.uint32)
    n = len(m)
    out = dict(material=np.zeros((n, 8)), color_raw=m[:, :3].copy(), max_emission=0.0, classes=0, class_part=np.zeros(n, np.uint32),
               emission_part=np.zeros(n), ok=np.zeros(n, bool), flags=f.copy())
    for i in range(n):
        c, e = [float(x) for x in m[i, :3]], [float(x) for x in m[i, 3:]]
        out["material"][i] = record(int(f[i]), c, e)
        out["class_part"][i] = class_part(int(f[i]))
        out["emission_part"][i] = emission_part(e)
        out["ok"][i] = material_ok(c, e)
        if out["ok"][i]:
            out["max_emission"] = max(out["max_emission"], out["emission_part"][i])
            out["classes"] |= int(out["class_part"][i])
    return out


def same_records(a, b):
    """float64 arrays: equal bits, or NaN on both sides"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))).all())


def same_bits(a, b):
    return np.float64(a).view(np.uint64) == np.float64(b).view(np.uint64)


def mismatch(got, want):
    """-> "" or what differs between the harness's result and expected()'s"""
    for f in ("material", "color_raw", "emission_part"):
        if not same_records(got[f], want[f]):
            return f"{f}: {got[f]!r} != {want[f]!r}"
    if not same_bits(got["max_emission"], want["max_emission"]):
        return f"max_emission {got['max_emission']!r} != {want['max_emission']!r}"
    for f in ("class_part", "ok", "flags"):
        if not np.array_equal(got[f], want[f]):
            return f"{f}: {got[f]} != {want[f]}"
    return "" if got["classes"] == want["classes"] else f"classes {got['classes']} != {want['classes']}"


def compile_harness(out_dir, extra=("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")):
    """g++ build of tests/material_harness.cpp as a stand-alone program, under AddressSanitizer and UBSan"""
    out = os.path.join(str(out_dir), "material_main")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off"] + list(extra) +
                   ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "raytracer.c_amd", "csrc"),
                    os.path.join(ROOT, "tests", "material_harness.cpp"), "-o", out], check=True)
    return out


def run_harness(prog, lists):
    """the program over `lists` of (materials (n, 6), flags (n,)) -> one dict per list, in expected()'s form"""
    text = []
    for m, f in lists:
        m = np.ascontiguousarray(m, dtype=np.float64).reshape(-1, 6)
        f = np.asarray(f).reshape(-1).astype(np.uint32)
        text.append("%d %s" % (len(m), " ".join(" ".join("%016x" % u for u in row.view(np.uint64)) + " %x" % fl for row, fl in zip(m, f))))
    out = subprocess.run([prog], input="\n".join(text) + "\n", capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = out.stdout.strip("\n").split("\n")
    assert len(lines) == len(lists)
    res = []

    def f64(words):
        return np.array([int(x, 16) for x in words], dtype=np.uint64).view(np.float64)
    for (m, _), line in zip(lists, lines):
        n, w = len(np.asarray(m).reshape(-1, 6)), line.split()
        assert len(w) == 11 * n + 2 + 4 * n
        per = w[11 * n + 2:]
        res.append(dict(material=f64(w[:8 * n]).reshape(n, 8), color_raw=f64(w[8 * n:11 * n]).reshape(n, 3),
                        max_emission=float(f64(w[11 * n:11 * n + 1])[0]), classes=int(w[11 * n + 1], 16),
                        class_part=np.array([int(x, 16) for x in per[0::4]], dtype=np.uint32), emission_part=f64(per[1::4]),
                        ok=np.array([x == "1" for x in per[2::4]], dtype=bool), flags=np.array([int(x, 16) for x in per[3::4]], dtype=np.uint32)))
    return res


# ---- a host scene's materials, in the shim's numbering ----
def _things(sc):
    return [sc.objects[i] for i in range(sc.n_objects)] + [sc.meshes[m] for m in range(sc.n_meshes)]


def materials_of(sc):
    """-> (colors (n, 3), emission (n, 3), flags (n,) uint32) of a host scene: spheres, then meshes"""
    t = _things(sc)
    return (np.array([o.color.tuple() for o in t], dtype=np.float64).reshape(-1, 3),
            np.array([o.emission.tuple() for o in t], dtype=np.float64).reshape(-1, 3), np.array([o.flags for o in t], dtype=np.uint32))


def set_materials(sc, colors, emission, flags):
    """writes them into the host scene: a scene created from it afterwards is the fresh scene of these materials"""
    from rt_amd import abi
    for i, o in enumerate(_things(sc)):
        o.color = abi.Vec3(*[float(x) for x in colors[i]])
        o.emission = abi.Vec3(*[float(x) for x in emission[i]])
        o.flags = int(flags[i])

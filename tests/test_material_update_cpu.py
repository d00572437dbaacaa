"""Material updates without a device: scene_materials.h (raytracer.c_amd/csrc), the one text of what a scene derives from its
materials, run as a stand-alone program under AddressSanitizer and UBSan (tests/material_harness.cpp) and compared bit for bit --
a NaN equal to a NaN -- with the scalar Python restatement (tests/material_expected.py): about 200 random materials and the edges
of every rule; and the C interface of the feature before any device is touched."""
import ctypes as C
import itertools

import numpy as np
import pytest

import material_expected as E

UP = np.nextafter
FLAG_SETS = [sum(c) for k in range(5) for c in itertools.combinations((E.M_DEFAULT, E.M_REFLECTION, E.M_REFRACTION, E.M_CHECKERED), k)]


def mats(rows, flags=None):
    m = np.array(rows, dtype=np.float64).reshape(-1, 6)
    return m, np.full(len(m), E.M_DEFAULT, np.uint32) if flags is None else np.array(flags, dtype=np.uint32)


def cases():
    rng = np.random.default_rng(28)
    n = 200
    rand = np.concatenate([rng.uniform(0, 1, (n, 3)) * rng.choice([1.0, 1.0, 3.0, 1e-9], (n, 1)),
                           rng.normal(size=(n, 3)) * rng.choice([0.0, 1.0, 40.0, 1e9], (n, 1))], axis=1)
    out = {"random": (rand, rng.choice(FLAG_SETS, n).astype(np.uint32)), "empty": mats([])}
    out["black"] = mats([[0, 0, 0, 0, 0, 0], [0.0, -0.0, 0.0, 1, 2, 3]])                       # prob 0: 0 * inf
    out["white_and_above"] = mats([[1, 1, 1, 0, 0, 0], [2.5, 1.0, 0.25, 0, 0, 0], [1e100, 1e99, 1.0, 0, 0, 0]])
    out["one_channel_zero"] = mats([[0, 0.5, 0.25, 0, 0, 0], [0.5, 0, 0.25, 0, 0, 0], [0.5, 0.25, 0, 0, 0, 0]])
    out["prob_by_each_channel"] = mats([[0.9, 0.2, 0.1, 0, 0, 0], [0.2, 0.9, 0.1, 0, 0, 0], [0.2, 0.1, 0.9, 0, 0, 0], [0.3, 0.3, 0.3, 0, 0, 0]])
    out["emission"] = mats([[0.5, 0.5, 0.5, 0, 0, 0], [0.5, 0.5, 0.5, 1e9, -1e9, 0], [0.5, 0.5, 0.5, -1e100, 0, 1e100],
                            [0.5, 0.5, 0.5, -0.0, 0.0, -0.0], [0.5, 0.5, 0.5, 3, -7, 5]])
    out["emission_zero_only"] = mats([[0.5, 0.5, 0.5, 0, -0.0, 0]] * 3)
    out["every_flag_set"] = (np.tile([0.6, 0.5, 0.4, 1.0, 0.0, 2.0], (16, 1)), np.array(FLAG_SETS, dtype=np.uint32))
    for k, f in enumerate(FLAG_SETS):
        out[f"flags_{f}"] = mats([[0.6, 0.5, 0.4, 0, 0, 0]], [f])
    out["high_flag_bits"] = mats([[0.6, 0.5, 0.4, 0, 0, 0]] * 2, [0xFFFFFFFF, 0x80000002])
    above = float(UP(1e100, np.inf))
    out["at_the_limit"] = mats([[1e100, 0, 0, 1e100, -1e100, 0], [-0.0, -0.0, -0.0, 0, 0, 0]])
    out["above_the_limit"] = mats([[above, 0, 0, 0, 0, 0], [0.5, 0.5, 0.5, above, 0, 0], [0.5, 0.5, 0.5, 0, -above, 0], [0.5, 0.5, 0.5, 2e100, 0, 0]])
    out["negative_colour"] = mats([[-1e-300, 0.5, 0.5, 0, 0, 0], [0.5, 0.5, -1.0, 0, 0, 0], [0.5, 0.5, 0.5, 4, 0, 0]])
    out["nan_and_inf"] = mats([[np.nan, 0.5, 0.5, 0, 0, 0], [0.5, np.inf, 0.5, 0, 0, 0], [0.5, 0.5, 0.5, np.nan, 0, 0],
                               [0.5, 0.5, 0.5, 0, -np.inf, 0], [0.5, 0.5, 0.5, 6, 0, 0]], [E.M_REFRACTION, E.M_CHECKERED, 12, 2, 2])
    return out


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    """the sanitized program, run once over every case"""
    c = cases()
    prog = E.compile_harness(tmp_path_factory.mktemp("materials"))
    return c, dict(zip(c, E.run_harness(prog, list(c.values()))))


@pytest.mark.parametrize("name", list(cases()))
def test_header_equals_the_scalar_restatement(results, name):
    c, got = results
    want = E.expected(*c[name])
    assert not E.mismatch(got[name], want), f"{name}: {E.mismatch(got[name], want)}"


def test_the_edges_fall_where_the_rules_say(results):
    c, got = results
    g = lambda k: got[k]
    r = g("random")
    assert r["ok"].all() and r["max_emission"] > 1e9 and r["classes"] == 7 and len(r["material"]) == 200
    assert np.array_equal(r["color_raw"], c["random"][0][:, :3]) and np.array_equal(r["material"][:, 4:7], c["random"][0][:, 3:])
    # black: prob 0, inv +inf, 0 * inf = NaN in the three albedo doubles; accepted all the same
    b = g("black")
    assert (b["material"][:, 0] == 0).all() and np.isnan(b["material"][:, 1:4]).all() and b["ok"].all() and b["max_emission"] == 3.0
    w = g("white_and_above")["material"]
    assert (w[0, :4] == 1.0).all() and w[1, 0] == 2.5 and w[1, 1] == 2.5 * (1 / 2.5) and w[1, 3] == 0.25 * (1 / 2.5) and w[2, 0] == 1e100
    z = g("one_channel_zero")["material"]
    assert (z[:, 0] == 0.5).all() and z[0, 1] == 0 and z[1, 2] == 0 and z[2, 3] == 0
    assert list(g("prob_by_each_channel")["material"][:, 0]) == [0.9, 0.9, 0.9, 0.3]
    e = g("emission")
    assert list(e["emission_part"]) == [0.0, 1e9, 1e100, 0.0, 7.0] and e["max_emission"] == 1e100
    assert np.signbit(e["material"][3, 4]) and not np.signbit(e["material"][3, 5]), "the emission is kept as given, -0.0 included"
    assert g("emission_zero_only")["max_emission"] == 0.0 and not np.signbit(g("emission_zero_only")["max_emission"])
    # the flag classes, for each of the sixteen sets of the four bits
    for f in FLAG_SETS:
        one = g(f"flags_{f}")
        want = (1 if f & 8 else 0) | (2 if f & 16 else 0) | (4 if f & 12 == 12 else 0)
        assert one["classes"] == want == one["class_part"][0] and one["flags"][0] == f, f
        assert one["material"][0, 7:].view(np.uint64)[0] == f, "the flags are the uint64 bit pattern of double 7"
    assert g("every_flag_set")["classes"] == 7 and g("flags_2")["classes"] == 0 and g("flags_0")["classes"] == 0
    assert list(g("high_flag_bits")["flags"]) == [0xFFFFFFFF, 0x80000002] and g("high_flag_bits")["material"][0, 7:].view(np.uint64)[0] == 0xFFFFFFFF
    # acceptance: at 1e100 and at -0.0 yes; just above, negative, NaN and infinite no -- and a refused object gives no scalar
    assert g("at_the_limit")["ok"].all() and g("at_the_limit")["max_emission"] == 1e100
    assert not g("above_the_limit")["ok"].any() and g("above_the_limit")["max_emission"] == 0.0
    assert list(g("negative_colour")["ok"]) == [False, False, True] and g("negative_colour")["max_emission"] == 4.0
    q = g("nan_and_inf")
    assert list(q["ok"]) == [False, False, False, False, True] and q["max_emission"] == 6.0 and q["classes"] == 0


def test_interface():
    """the symbols in both builds of the shim and in the host library, abi.py against the headers, the switch's default, and the
    argument errors that need no device"""
    import os
    import re
    from rt_amd import abi
    shim, host = abi.load_shim(), abi.load_host()
    names = ("rt_hip_scene_update_materials", "rt_hip_scene_update_materials_host", "rt_hip_scene_read_materials",
             "rt_hip_scene_material_bounds", "rt_hip_scene_memory", "rt_hip_set_material_updates")
    diag = C.CDLL(os.path.join(os.path.dirname(abi.SHIM_PATH), "librt_hip_diag.so"))
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(E.ROOT, "include", "rt_hip.h")).read(), flags=re.S)
    for name in names:
        assert hasattr(shim, name) and hasattr(diag, name), name
        assert name in abi.SHIM_SYMBOLS and re.search(r"\b%s\s*\(" % name, header), name
    host_header = re.sub(r"/\*.*?\*/", "", open(os.path.join(E.ROOT, "include", "raytracer.h")).read(), flags=re.S)
    for name in ("rt_set_material_updates", "rt_get_material_updates"):
        assert hasattr(host, name) and re.search(r"\b%s\s*\(" % name, host_header), name
    assert host.rt_get_material_updates() == 0, "the default keeps today's behaviour"
    before = shim.rt_hip_cache_updates()
    host.rt_set_material_updates(5)
    assert host.rt_get_material_updates() == 1
    host.rt_set_material_updates(0)
    assert host.rt_get_material_updates() == 0 and shim.rt_hip_cache_updates() == before
    buf, flags = (C.c_double * 12)(), (C.c_uint32 * 2)()
    assert shim.rt_hip_scene_update_materials(None, buf, flags, 2) == abi.EINVAL
    assert shim.rt_hip_scene_update_materials_host(None, buf, None, 2) == abi.EINVAL
    assert shim.rt_hip_scene_update_materials_host(None, None, None, 2) == abi.EINVAL and b"required" in shim.rt_hip_last_error()
    assert shim.rt_hip_scene_read_materials(None, None, None) == abi.EINVAL
    assert shim.rt_hip_scene_material_bounds(None, None, None, None, None) == abi.EINVAL
    assert shim.rt_hip_scene_memory(None, None, None) == abi.EINVAL

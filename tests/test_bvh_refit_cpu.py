"""BvhRefit (raytracer.c_amd/csrc/bvh_build.h), the sequential statement of a refit to moved triangles, on the CPU: unchanged
geometry reproduces the tree (bytes on BvhSweep's, values on BvhBuild's, whose fmin leaves the sign of a zero open), deformed
geometry gives at every child the numpy join of its range's triangle boxes with refs, order and the empty child untouched, the
levels the device sweeps are a partition of the nodes with children one level below their parents, and the harness runs clean as
a stand-alone program under AddressSanitizer and UBSan.  Then the C interface of the feature before any device is touched."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import bvh_sweep_meshes as M
import scene_update_meshes as U

NAMES = [k for k in M.MESHES if k != "n300000"]      # every mesh up to n65537


@pytest.fixture(scope="module")
def refit(tmp_path_factory):
    return U.Refit(U.compile_harness(tmp_path_factory.mktemp("refit")))


@pytest.mark.parametrize("name", NAMES)
def test_unchanged_geometry_reproduces_the_sweep_tree(refit, name):
    g = M.geom(M.mesh(name))
    nodes, order = refit.build("device", g)
    again = refit.refit(nodes, order, g)
    assert np.array_equal(again.view(np.uint64), nodes.view(np.uint64)), f"{name}: {(again != nodes).any(axis=1).sum()} nodes differ"
    if name == "n1":
        assert M.node_refs(nodes)[0, 1] == M.LEAF_FLAG, "the empty second child"


@pytest.mark.parametrize("name", NAMES)
def test_unchanged_geometry_reproduces_the_host_tree(refit, name):
    g = M.geom(M.mesh(name))
    nodes, order = refit.build("host", g)
    again = refit.refit(nodes, order, g)
    assert np.array_equal(again[:, 12:].view(np.uint64), nodes[:, 12:].view(np.uint64)), "refs and padding are byte-equal"
    assert (again[:, :12] == nodes[:, :12]).all(), "every box double equals the original (the sign of a zero may differ)"


@pytest.mark.parametrize("builder", list(U.BUILDERS))
@pytest.mark.parametrize("deform", list(U.DEFORMATIONS))
@pytest.mark.parametrize("name", ["n1", "n16", "n17", "n241", "n257", "duplicated", "signed_zeros", "flat", "uv_sphere"])
def test_deformed_geometry(refit, name, deform, builder):
    tris = M.mesh(name)
    nodes, order = refit.build(builder, M.geom(tris))
    g = M.geom(U.DEFORMATIONS[deform](tris))
    out = refit.refit(nodes, order, g)
    U.check_refitted(nodes, order, out, g, f"{name} {deform} {builder}")
    # a second refit of the result to the same triangles changes nothing: the result does not depend on what the boxes held
    assert np.array_equal(refit.refit(out, order, g).view(np.uint64), out.view(np.uint64))
    if deform == "squash":   # and back: the device tree's bytes return
        back = refit.refit(out, order, M.geom(tris))
        if builder == "device":
            assert np.array_equal(back.view(np.uint64), nodes.view(np.uint64))
        else:
            assert (back[:, :12] == nodes[:, :12]).all()


@pytest.mark.parametrize("builder", list(U.BUILDERS))
@pytest.mark.parametrize("name", ["n1", "n17", "n257", "uv_sphere"])
def test_levels(refit, name, builder):
    nodes, _ = refit.build(builder, M.geom(M.mesh(name)))
    by_level, begin = refit.levels(nodes)
    assert sorted(by_level.tolist()) == list(range(len(nodes))) and begin[0] == 0 and begin[-1] == len(nodes)
    depth = np.zeros(len(nodes), dtype=np.int64)
    for d in range(len(begin) - 1):
        assert begin[d + 1] > begin[d]
        depth[by_level[begin[d]:begin[d + 1]]] = d
    refs = M.node_refs(nodes)
    for k in range(len(nodes)):
        for r in refs[k]:
            if not r & M.LEAF_FLAG:
                assert r > k and depth[r] == depth[k] + 1
    assert by_level[0] == 0


def test_sanitized_program(tmp_path):
    """the harness as a stand-alone program under AddressSanitizer and UBSan, once over n17, n257 and uv_sphere"""
    prog = U.compile_harness(tmp_path, extra=["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], program=True)
    files = []
    for name in ("n17", "n257", "uv_sphere"):
        files.append(str(tmp_path / f"{name}.f64"))
        M.geom(M.mesh(name)).tofile(files[-1])
    out = subprocess.run([prog] + files, capture_output=True, text=True)
    assert out.returncode == 0 and "refit ok" in out.stdout, out.stdout + out.stderr


def test_interface():
    """the symbols, and the argument errors that come before any device is looked at"""
    from rt_amd import abi
    shim, host = abi.load_shim(), abi.load_host()
    for name in ("rt_hip_scene_update_vertices", "rt_hip_scene_update_vertices_host", "rt_hip_scene_update_info",
                 "rt_hip_scene_read_triangles", "rt_hip_scene_bounds", "rt_hip_set_scene_updates", "rt_hip_cache_updates"):
        assert hasattr(shim, name)
    buf = (C.c_double * 9)()
    assert shim.rt_hip_scene_update_vertices(None, buf, 1) == abi.EINVAL
    assert shim.rt_hip_scene_update_vertices_host(None, buf, 1) == abi.EINVAL and b"required" in shim.rt_hip_last_error()
    assert shim.rt_hip_scene_update_info(None, None, None) == abi.EINVAL
    assert shim.rt_hip_scene_read_triangles(None, None, None, None, None) == abi.EINVAL
    assert shim.rt_hip_scene_bounds(None, None, None, None, None) == abi.EINVAL
    assert host.rt_get_scene_updates() == 0, "the default keeps today's behaviour"
    before = shim.rt_hip_cache_updates()
    host.rt_set_scene_updates(1)
    assert host.rt_get_scene_updates() == 1
    host.rt_set_scene_updates(0)
    assert host.rt_get_scene_updates() == 0 and shim.rt_hip_cache_updates() == before

"""The device cost of a tree and the in-place rebuild, without a GPU (include/rt_hip.h: rt_hip_scene_bvh_cost,
rt_hip_scene_rebuild_bvh, rt_hip_scene_maintain_bvh):
  1. the numpy restatement of the cost contract (tests/bvh_cost_expected.py) equals a scalar Python loop of the same contract bit for
     bit, at the block and level edges of the reduction and on every totality case;
  2. it stays within n_nodes * 2^-52 * cost of the sequential BvhBuild::tree_cost() (tests/bvh_sweep_harness.cpp) on the meshes of
     tests/bvh_sweep_meshes.py.  The bound is derived, not observed: both are sums of the same 2 n_nodes non-negative terms, so
     nothing cancels; the sequential sum S of N = 2 n_nodes + 1 addends (60 first) errs by at most (N - 1) u S = n_nodes 2^-52 S to
     first order, u = 2^-53, and the fixed tree's own error -- at most its depth, 8 a level, times u S -- is what the bound
     neglects beside it.  Every mesh of the file is run, n300000 with its 28,000 nodes included; every case prints its
     observed share of the bound and the worst share so far, so the last line is the worst over all;
  3. totality: NaN and infinite boxes, roots without an area, the one-leaf root with its empty second child;
  4. the interface: every build of the shim exports the new entry points, abi.py agrees with the header, and the argument errors
     that need no device come out as the header says, RT_HIP_EINVAL before RT_HIP_ENODEV;
  5. the two committed pairs of position sets: BvhSweep's trees differ in node count the way their names say, so the GPU test that
     rebuilds from one to the other crosses the node capacity; and the committed climb has ever more nodes, so its second rebuild
     replaces a side allocation by a larger one;
  6. the C host carries the rebuild ratio (include/raytracer.h): default 0, set, get, a bad value ignored."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import bvh_cost_expected as E
import bvh_sweep_meshes as M
import scene_update_meshes as U

ROOT = M.ROOT
NEW_SYMBOLS = ["rt_hip_scene_bvh_cost", "rt_hip_bvh_cost_nodes_host", "rt_hip_scene_rebuild_bvh", "rt_hip_scene_rebuild_info",
               "rt_hip_scene_maintain_bvh", "rt_hip_set_bvh_rebuild_ratio", "rt_hip_cache_rebuilds"]


@pytest.fixture(scope="module")
def sweep(tmp_path_factory):
    return M.Sweep(M.compile_harness(tmp_path_factory.mktemp("sweep")))


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 511, 513, 65537])
def test_numpy_restatement_equals_the_scalar_loop(n):
    nodes = E.synthetic_nodes(n)
    a, b = E.cost(nodes), E.cost_scalar(nodes)
    assert np.isfinite(a) and a > 60.0
    assert E.same_cost(a, b), f"{n} nodes: numpy {a!r}, the scalar loop {b!r}"


def test_the_fixed_tree_is_not_the_sequential_sum():
    """the restatement would pass every comparison with itself if it summed in node order: here the two orders differ"""
    t = E.terms(E.synthetic_nodes(65537), E.root_area(E.synthetic_nodes(65537)))
    seq = 0.0
    for x in t.tolist():
        seq += x
    assert E.tree_sum(t) != seq and abs(E.tree_sum(t) - seq) <= len(t) * 2.0 ** -52 * seq


def test_totality():
    cases = E.totality_cases()
    got = {}
    for name, nodes in cases.items():
        a, b = E.cost(nodes), E.cost_scalar(nodes)
        assert E.same_cost(a, b), f"{name}: numpy {a!r}, the scalar loop {b!r}"
        got[name] = a
    for name in ("nan_root", "inf_root", "huge_root", "zero_area_root", "flat_root", "inverted_root"):
        assert got[name] == 0.0 and not np.signbit(got[name]), f"{name}: {got[name]!r}"
    assert np.isnan(got["nan_child_box"]) and np.isnan(got["inf_minus_inf"])
    assert got["inf_child_box"] == np.inf
    for name in ("nan_in_one_root_box", "inverted_child_box", "garbage_refs"):
        assert np.isfinite(got[name]), f"{name}: {got[name]!r}"
    base = E.synthetic_nodes(300, E.SEED + 1)
    assert got["padding_ignored"] == E.cost(base)
    # the one-leaf root: its leaf fills the root's box, so the cost is the root's visit and the leaf's seven pre-tests
    assert got["one_leaf_root"] == 60.0 + 45.0 * 7
    assert E.cost(np.zeros((0, 16))) == 0.0


SHARES = {}      # mesh -> |fixed - sequential| / bound, for the report of the worst


@pytest.mark.parametrize("name", list(M.MESHES))
def test_within_the_derived_bound_of_the_sequential_cost(sweep, name):
    r = sweep.build(M.geom(M.mesh(name)))
    assert r["rc"] == 0
    seq, fixed = r["cost"], E.cost(r["nodes"])
    if not np.isfinite(seq) or seq == 0.0:
        assert E.same_cost(seq, fixed), f"{name}: sequential {seq!r}, fixed tree {fixed!r}"
        return
    bound = r["n_nodes"] * 2.0 ** -52 * seq
    print(f"{name}: {r['n_nodes']} nodes, cost {seq!r}, |fixed - sequential| = {abs(fixed - seq):.3e} = {abs(fixed - seq) / bound:.3f} of the bound")
    SHARES[name] = abs(fixed - seq) / bound
    worst = max(SHARES, key=SHARES.get)      # the last case's line is the report over all meshes
    print(f"worst share of the bound over the {len(SHARES)} meshes so far: {SHARES[worst]:.4f} ({worst})")
    assert abs(fixed - seq) <= bound


def test_host_library_carries_the_ratio():
    """rt_set_bvh_rebuild_ratio / rt_get_bvh_rebuild_ratio (include/raytracer.h): the default 0, set, get, a bad value ignored"""
    from rt_amd import abi
    shim, host = abi.load_shim(), abi.load_host()
    header = open(os.path.join(ROOT, "include", "raytracer.h")).read()
    assert "rt_set_bvh_rebuild_ratio" in header and "rt_get_bvh_rebuild_ratio" in header
    assert host.rt_get_bvh_rebuild_ratio() == 0.0, "the default never rebuilds"
    before = shim.rt_hip_cache_rebuilds()
    host.rt_set_bvh_rebuild_ratio(1.25)
    assert host.rt_get_bvh_rebuild_ratio() == 1.25
    for bad in (float("nan"), 0.5, -1.0, float("inf")):
        host.rt_set_bvh_rebuild_ratio(bad)
        assert host.rt_get_bvh_rebuild_ratio() == 1.25, f"{bad} must leave the setting"
    host.rt_set_bvh_rebuild_ratio(0.0)
    assert host.rt_get_bvh_rebuild_ratio() == 0.0 and shim.rt_hip_cache_rebuilds() == before


def test_interface():
    from rt_amd import abi
    header = open(os.path.join(ROOT, "include", "rt_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} is not declared in rt_hip.h"
        assert name in abi.SHIM_SYMBOLS, f"{name} has no binding in abi.py"
    assert "recreate the scene when it has drifted too far" not in header
    csrc = os.path.join(ROOT, "raytracer.c_amd", "csrc")
    for lib in ("librt_hip.so", "librt_hip_dev.so", "librt_hip_diag.so"):
        out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(csrc, lib)], capture_output=True, text=True, check=True).stdout
        exported = set(re.findall(r"\bT (rt_hip_\w+)", out))
        assert set(NEW_SYMBOLS) <= exported, f"{lib}: {sorted(set(NEW_SYMBOLS) - exported)} not exported"


def test_argument_errors_need_no_device():
    from rt_amd import abi
    shim = abi.load_shim()
    cost, ratio, rebuilt, k = C.c_double(7.0), C.c_double(7.0), C.c_int(7), C.c_uint64(7)
    assert shim.rt_hip_scene_bvh_cost(None, C.byref(cost)) == abi.EINVAL
    assert shim.rt_hip_scene_rebuild_bvh(None) == abi.EINVAL
    assert b"NULL" in shim.rt_hip_last_error()
    assert shim.rt_hip_scene_rebuild_info(None, C.byref(k), None, None) == abi.EINVAL
    assert shim.rt_hip_scene_maintain_bvh(None, 1.5, C.byref(ratio), C.byref(rebuilt)) == abi.EINVAL
    assert (ratio.value, rebuilt.value) == (0.0, 0)
    for bad in (float("nan"), 0.5, 0.0, -2.0, float("inf")):        # the ratio is checked before the scene
        assert shim.rt_hip_scene_maintain_bvh(None, bad, None, None) == abi.EINVAL
        assert b"max_ratio" in shim.rt_hip_last_error(), bad
    nodes = E.synthetic_nodes(5)
    no_device = 9999                                              # no machine has it: the answer is the same with and without a GPU
    assert shim.rt_hip_bvh_cost_nodes_host(None, 5, no_device, C.byref(cost)) == abi.EINVAL
    assert shim.rt_hip_bvh_cost_nodes_host(nodes.ctypes.data, 5, no_device, None) == abi.EINVAL
    assert shim.rt_hip_bvh_cost_nodes_host(nodes.ctypes.data, 1 << 27, no_device, C.byref(cost)) == abi.EINVAL
    assert shim.rt_hip_bvh_cost_nodes_host(nodes.ctypes.data, 5, no_device, C.byref(cost)) == abi.ENODEV
    assert cost.value == 0.0
    cost.value = 7.0
    assert shim.rt_hip_bvh_cost_nodes_host(None, 0, no_device, C.byref(cost)) == 0 and cost.value == 0.0     # no nodes, no device needed
    r0 = shim.rt_hip_cache_rebuilds()
    for bad in (float("nan"), 0.5, -1.0, float("inf")):
        assert shim.rt_hip_set_bvh_rebuild_ratio(bad) == abi.EINVAL
    assert shim.rt_hip_set_bvh_rebuild_ratio(1.25) == 0 and shim.rt_hip_set_bvh_rebuild_ratio(0.0) == 0
    assert shim.rt_hip_cache_rebuilds() == r0


@pytest.mark.parametrize("name", list(E.PAIRS))
def test_committed_pairs_differ_in_node_count(tmp_path_factory, name):
    refit = U.Refit(U.compile_harness(tmp_path_factory.mktemp("refit")))
    a, b = E.pair(name)
    assert a.shape == b.shape and len(a) <= 400
    na, nb = (len(refit.build("device", M.geom(t))[0]) for t in (a, b))
    print(f"{name}: {len(a)} triangles, {na} -> {nb} nodes")
    assert nb > na if name == "grows" else nb < na


def test_committed_climb_has_ever_more_nodes(tmp_path_factory):
    refit = U.Refit(U.compile_harness(tmp_path_factory.mktemp("refit")))
    counts = [len(refit.build("device", M.geom(t))[0]) for t in E.climb()]
    print(f"climb: {counts} nodes")
    assert counts[0] < counts[1] < counts[2]

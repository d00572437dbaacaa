"""BvhSweep (raytracer.c_amd/csrc/bvh_build.h), the sequential statement of the tree the device builder makes, on the CPU:
its invariants over the mesh set, its splits against a numpy sweep written from the contract's text, its quality against the
host builder's tree, and the C interface of the feature before any device is touched."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import bvh_sweep_meshes as M


@pytest.fixture(scope="module")
def sweep(tmp_path_factory):
    return M.Sweep(M.compile_harness(tmp_path_factory.mktemp("sweep")))


@pytest.mark.parametrize("name", list(M.MESHES))
def test_invariants(sweep, name):
    """order is a permutation, the leaves tile it, no leaf above 15, depth <= max_depth = the least depth, every child box is
    bit for bit the min / max of its members, two builds agree (the harness's return codes say which one failed)"""
    g = M.geom(M.mesh(name))
    r = sweep.build(g)
    assert r["rc"] == 0, f"{name}: invariant {r['rc']} violated"
    n, least = len(g), 0
    while M.LEAF * 2 ** least < n:
        least += 1
    assert r["max_depth"] == least and r["depth"] <= max(least, 1)
    assert r["n_nodes"] == max(r["leaves"] - 1, 1) and r["leaves"] * M.LEAF >= n
    assert sorted(r["order"].tolist()) == list(range(n))
    if n == 240:   # zero slack: only i = m / 2 is admissible at every level, so the tree is complete and every leaf holds 15
        assert r["n_nodes"] == 15 and (r["left"] * 2 == np.diff(M.node_ranges(r["nodes"])[0], axis=1)[:, 0]).all()


def _half_area(lo, hi):
    d = hi - lo
    return d[..., 0] * d[..., 1] + d[..., 1] * d[..., 2] + d[..., 2] * d[..., 0]


def _numpy_split(box, cen, members, cap):
    """the contract's split search over one range, from its text: -> (axis, i, the winner list's first i members)"""
    m = len(members)
    best, best_axis, best_i, best_list = np.inf, 0, m // 2, None
    lists = []
    for a in range(3):
        ids = members[np.lexsort((members, cen[members, a] + 0.0))]        # by (cen[a] + 0.0, index)
        lists.append(ids)
        lo, hi = box[ids, :3], box[ids, 3:]
        al = _half_area(np.minimum.accumulate(lo, axis=0), np.maximum.accumulate(hi, axis=0))            # box of the first j + 1
        ar = _half_area(np.minimum.accumulate(lo[::-1], axis=0)[::-1], np.maximum.accumulate(hi[::-1], axis=0)[::-1])  # of [j, m)
        i = np.arange(1, m)
        with np.errstate(invalid="ignore", over="ignore"):
            cost = al[i - 1] * i.astype(np.float64) + ar[i] * (m - i).astype(np.float64)
        cost = np.where((i <= cap) & (m - i <= cap) & ~np.isnan(cost), cost, np.inf)
        k = int(np.argmin(cost))                                             # the first of equal costs: the lower i
        if cost[k] < best:                                                   # strictly: ties go to the lower axis
            best, best_axis, best_i = cost[k], a, int(i[k])
    return best_axis, best_i, lists[best_axis][:best_i], best


@pytest.mark.parametrize("name", [k for k in M.MESHES if k.startswith("n") and int(k[1:]) <= 257] +
                         ["duplicated", "same_centroid", "flat", "signed_zeros", "huge", "nan_area", "shell3000"])
def test_contract(sweep, name):
    """every node's (axis, i) equals the one a direct numpy sweep over the node's members finds, and the node's left child holds
    exactly the winner list's first i members; on the meshes with infinite and NaN areas, nodes keep the starting winner"""
    g = M.geom(M.mesh(name))
    r = sweep.build(g)
    assert r["rc"] == 0
    if len(g) <= M.LEAF:
        assert r["n_nodes"] == 1 and r["depth"] == 1 and M.node_refs(r["nodes"])[0, 1] == M.LEAF_FLAG
        return
    a, b, c = g[:, 0:3], g[:, 0:3] + g[:, 3:6], g[:, 0:3] + g[:, 6:9]
    box = np.concatenate([np.minimum(a, np.minimum(b, c)), np.maximum(a, np.maximum(b, c))], axis=1)
    cen = (a + b + c) / 3.0
    ranges, child = M.node_ranges(r["nodes"])
    level = {0: 0}
    refs = M.node_refs(r["nodes"])
    for k in range(r["n_nodes"]):
        for ref in refs[k]:
            if not ref & M.LEAF_FLAG:
                level[int(ref)] = level[k] + 1
    assert sorted(level) == list(range(r["n_nodes"])) and all(level[k] <= level[k + 1] for k in range(r["n_nodes"] - 1)), \
        "nodes are numbered level by level"
    kept_start = 0   # nodes where no cost was finite: the starting winner (axis 0, m / 2) stood
    for k in range(r["n_nodes"]):
        b0, e0 = ranges[k]
        members = np.sort(r["order"][b0:e0]).astype(np.int64)
        cap = M.LEAF << (r["max_depth"] - level[k] - 1)
        axis, i, left, cost = _numpy_split(box, cen, members, cap)
        if cost == np.inf:
            assert (axis, i) == (0, (e0 - b0) // 2)
            kept_start += 1
        assert (axis, i) == (int(r["axis"][k]), int(r["left"][k])), f"{name}: node {k} of {e0 - b0}"
        assert child[k, 0, 1] - b0 == i
        assert sorted(left.tolist()) == sorted(r["order"][b0:b0 + i].tolist())
    if name in ("huge", "nan_area"):   # every node on the path to the one enormous triangle
        assert kept_start >= 2, f"{name}: {kept_start} nodes kept the starting winner at an infinite cost"
    else:
        assert kept_start == 0


def test_quality(sweep):
    """tree_cost(BvhSweep) <= 1.10 x tree_cost(BvhBuild::build_root) on the five meshes the bound was set on"""
    ratios = {}
    for name in M.QUALITY:
        g = M.geom(M.mesh(name))
        r = sweep.build(g)
        assert r["rc"] == 0
        ratios[name] = r["cost"] / sweep.host_cost(g)
        print(f"{name}: sweep {r['cost']:.3f} / host = {ratios[name]:.4f}")
    assert all(v <= 1.10 for v in ratios.values()), ratios


def test_sanitized_program(tmp_path):
    """the harness as a stand-alone program under AddressSanitizer and UBSan, over generators of its own"""
    prog = M.compile_harness(tmp_path, extra=["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], program=True)
    out = subprocess.run([prog], capture_output=True, text=True)
    assert out.returncode == 0 and "sweep ok" in out.stdout, out.stdout + out.stderr


def test_interface():
    """the symbols, the options struct, and the argument errors that come before any device is looked at"""
    from rt_amd import abi
    shim, host = abi.load_shim(), abi.load_host()
    for name in ("rt_hip_scene_options_defaults", "rt_hip_scene_create_opts", "rt_hip_scene_bvh_info", "rt_hip_scene_bvh_read",
                 "rt_hip_scene_bvh_build_seconds", "rt_hip_set_bvh_builder"):
        assert hasattr(shim, name)
    assert hasattr(host, "rt_set_bvh_builder") and host.rt_get_bvh_builder() == 0
    assert C.sizeof(abi.RtHipSceneOptions) == 8
    opts = abi.RtHipSceneOptions()
    shim.rt_hip_scene_options_defaults(C.byref(opts))
    assert (opts.struct_size, opts.bvh_builder) == (8, abi.BVH_HOST), "the default is the host builder"
    handle = C.c_void_p(1)
    sphere = (abi.Object * 1)()
    sphere[0].radius = 1.0
    sphere[0].flags = abi.M_DEFAULT

    def create(o):
        return shim.rt_hip_scene_create_opts(sphere, 1, None, 0, 0, C.byref(o) if o is not None else None, C.byref(handle))

    bad = abi.RtHipSceneOptions(struct_size=4, bvh_builder=0)
    assert create(bad) == abi.EINVAL and b"struct_size" in shim.rt_hip_last_error() and not handle.value
    bad = abi.RtHipSceneOptions(struct_size=8, bvh_builder=2)
    assert create(bad) == abi.EINVAL and b"bvh_builder" in shim.rt_hip_last_error()
    assert shim.rt_hip_set_bvh_builder(2) == abi.EINVAL and shim.rt_hip_set_bvh_builder(-1) == abi.EINVAL
    assert shim.rt_hip_set_bvh_builder(1) == 0 and shim.rt_hip_set_bvh_builder(0) == 0
    host.rt_set_bvh_builder(7)
    assert host.rt_get_bvh_builder() == 0, "an unknown builder is ignored"
    assert shim.rt_hip_scene_bvh_info(None, None, None, None, None, None) == abi.EINVAL
    assert shim.rt_hip_scene_bvh_read(None, None, None) == abi.EINVAL
    if shim.rt_hip_device_count() < 1:
        # with valid options the call goes on to the device, as rt_hip_scene_create does: the same refusal from both
        plain = shim.rt_hip_scene_create(sphere, 1, None, 0, 0, C.byref(handle))
        assert create(opts) == plain == abi.ENODEV and create(None) == abi.ENODEV

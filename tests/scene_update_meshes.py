"""What the tests of a deforming mesh share (tests/test_bvh_refit_cpu.py, tests/test_gpu_scene_update.py): the deformations, the g++
build of tests/bvh_refit_harness.cpp (BvhRefit and the two builders through ctypes), and the numpy statement of a refitted tree's
boxes.  A mesh is an (n, 3, 3) float64 array of triangle corners, as in tests/bvh_sweep_meshes.py."""
import ctypes as C
import os
import subprocess

import numpy as np

import bvh_sweep_meshes as M

ROOT = M.ROOT
BUILDERS = {"host": 0, "device": 1}     # refit_build's builder: BvhBuild, BvhSweep


# ---- the deformations: (n, 3, 3) -> (n, 3, 3) ----
def identity(t):
    return np.array(t, dtype=np.float64)


def scale_wobble(t, phase=0.0):
    """scale 1.3 about (0.3, -0.2, 0.1) plus a sine wobble of 5 % of the extent (along each axis, driven by the next one)"""
    t = np.asarray(t, dtype=np.float64)
    c = np.array([0.3, -0.2, 0.1])
    flat = t.reshape(-1, 3)
    ext = float((flat.max(axis=0) - flat.min(axis=0)).max())
    ext = ext if ext > 0 else 1.0
    return c + 1.3 * (t - c) + 0.05 * ext * np.sin(2.0 * np.pi * np.roll(t, -1, axis=2) / ext + phase)


def mirror(t):
    """x -> -x, which reverses the order the tree was sorted in; v1 and v2 exchanged so that the normals stay outward"""
    t = np.array(t, dtype=np.float64)
    t[:, :, 0] = -t[:, :, 0]
    return np.ascontiguousarray(t[:, [0, 2, 1], :])


def squash(t):
    t = np.array(t, dtype=np.float64)
    t[:, :, 2] *= 0.05
    return t


def translate(t):
    """by 40 units, away from the camera of mesh_scene()"""
    return np.asarray(t, dtype=np.float64) + np.array([0.0, 0.0, -40.0])


DEFORMATIONS = {"identity": identity, "scale_wobble": scale_wobble, "mirror": mirror, "squash": squash, "translate": translate}


# ---- BvhRefit through the harness ----
def compile_harness(out_dir, extra=(), program=False):
    """g++ build of tests/bvh_refit_harness.cpp, the way tests/bvh_sweep_harness.cpp is built: the shared library, or with
    program=True the stand-alone program"""
    out = os.path.join(str(out_dir), "refit_main" if program else "libbvh_refit.so")
    kind = ["-DREFIT_MAIN"] if program else ["-shared", "-fPIC", "-Wl,-Bsymbolic"]
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off"] + kind + list(extra) +
                   ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "raytracer.c_amd", "csrc"),
                    os.path.join(ROOT, "tests", "bvh_refit_harness.cpp"), "-o", out], check=True)
    return out


class Refit:
    def __init__(self, so):
        self.lib = C.CDLL(so)
        self.lib.refit_build.restype = C.c_uint32
        self.lib.refit_build.argtypes = [C.c_int, C.c_void_p, C.c_uint32]
        self.lib.refit_fetch.restype = None
        self.lib.refit_fetch.argtypes = [C.c_void_p, C.c_void_p]
        self.lib.refit_apply.restype = C.c_int
        self.lib.refit_apply.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
        self.lib.refit_levels.restype = C.c_uint32
        self.lib.refit_levels.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]

    def build(self, builder, g):
        """-> (nodes (n_nodes, 16), order) of BvhBuild ("host") or BvhSweep ("device") over g = M.geom(tris)"""
        nn = self.lib.refit_build(BUILDERS[builder], g.ctypes.data, len(g))
        nodes, order = np.zeros((nn, M.SRC_DOUBLES)), np.zeros(len(g), dtype=np.uint32)
        self.lib.refit_fetch(nodes.ctypes.data, order.ctypes.data)
        return nodes, order

    def refit(self, nodes, order, g):
        """BvhRefit::refit of a copy of `nodes` to the triangles g -> the refitted nodes"""
        out = np.array(nodes, dtype=np.float64, order="C")
        order = np.ascontiguousarray(order, dtype=np.uint32)
        g = np.ascontiguousarray(g, dtype=np.float64)
        assert self.lib.refit_apply(out.ctypes.data, len(out), order.ctypes.data, g.ctypes.data) == 0, "a child numbered below its parent"
        return out

    def levels(self, nodes):
        nodes = np.ascontiguousarray(nodes)
        by_level, begin = np.zeros(len(nodes), dtype=np.uint32), np.zeros(len(nodes) + 2, dtype=np.uint32)
        n = self.lib.refit_levels(nodes.ctypes.data, len(nodes), by_level.ctypes.data, begin.ctypes.data)
        assert n > 0
        return by_level, begin[:n + 1]


def tri_boxes(g):
    """(n, 6) lo xyz hi xyz of the triangles g (n, 9: v0, e1, e2), by bvh_tri_box's expressions (values: numpy's minimum does not
    order the zeros)"""
    a, b, c = g[:, 0:3], g[:, 0:3] + g[:, 3:6], g[:, 0:3] + g[:, 6:9]
    return np.concatenate([np.minimum(a, np.minimum(b, c)), np.maximum(a, np.maximum(b, c))], axis=1)


def boxes_by_range(nodes, order, g):
    """the numpy statement: (n_nodes, 2, 6) -- every child's box as the join of the triangle boxes of its range of the leaf order
    (M.node_ranges); (+inf, -inf) for an empty child"""
    box = tri_boxes(g)[order]
    _, child = M.node_ranges(nodes)
    out = np.empty((len(nodes), 2, 6))
    out[:, :, :3], out[:, :, 3:] = np.inf, -np.inf
    for k in range(len(nodes)):
        for c in range(2):
            b, e = child[k, c]
            if e > b:
                out[k, c, :3] = box[b:e, :3].min(axis=0)
                out[k, c, 3:] = box[b:e, 3:].max(axis=0)
    return out


def check_refitted(nodes_before, order, refitted, g, what):
    """refs, padding and the empty child untouched; every other child box equals the numpy join of its range, by value"""
    assert np.array_equal(refitted[:, 12:].view(np.uint64), nodes_before[:, 12:].view(np.uint64)), f"{what}: refs or padding changed"
    want = boxes_by_range(refitted, order, g)
    have = refitted[:, :12].reshape(-1, 2, 6)
    _, child = M.node_ranges(refitted)
    empty = child[:, :, 1] == child[:, :, 0]
    assert empty.sum() == (1 if len(order) <= M.LEAF else 0), what
    assert np.array_equal(have[empty].view(np.uint64), nodes_before[:, :12].reshape(-1, 2, 6)[empty].view(np.uint64)), \
        f"{what}: the empty child was written"
    bad = np.nonzero((have != want)[~empty].any(axis=1))[0]
    assert bad.size == 0, f"{what}: {bad.size} child boxes differ from the join of their ranges"

"""The meshes the sweep builder is tested on (tests/test_bvh_sweep_cpu.py, tests/test_gpu_bvh_device.py), and the g++ build of
tests/bvh_sweep_harness.cpp, BvhSweep's checker.  A mesh is an (n, 3, 3) float64 array of triangle corners; geom() turns it into the
builder's input (v0, e1, e2).  Each is the smallest shape at which one mechanism of the builder can break."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEAF = 15            # PT_BVH_LEAF
SRC_DOUBLES = 16     # PT_BVH_SRC_DOUBLES
COUNT_BITS = 4       # PT_BVH_COUNT_BITS
LEAF_FLAG = 0x80000000


def shell(n, seed, size=0.02):
    """random thin triangles on the unit sphere"""
    rng = np.random.default_rng(seed)
    c = rng.normal(size=(n, 1, 3))
    c /= np.linalg.norm(c, axis=2, keepdims=True)
    return c + rng.normal(size=(n, 3, 3)) * size


def uv_sphere(rings=64, segs=80, r=8.0):
    """config 5's kind of mesh: rings x segs x 2 triangles"""
    t = np.linspace(0, np.pi, rings + 1)[:, None]
    p = np.linspace(0, 2 * np.pi, segs + 1)[None, :]
    v = r * np.stack([np.sin(t) * np.cos(p), np.cos(t) * np.ones_like(p), np.sin(t) * np.sin(p)], axis=-1)
    a, b, c, d = v[:-1, :-1], v[1:, :-1], v[1:, 1:], v[:-1, 1:]
    return np.concatenate([np.stack([a, b, c], axis=-2).reshape(-1, 3, 3), np.stack([a, c, d], axis=-2).reshape(-1, 3, 3)])


def cluster():
    """a dense cluster of 4,000 inside 1,000 sparse ones"""
    rng = np.random.default_rng(11)
    dense = np.array([0.3, 0.2, -0.1]) + rng.normal(size=(4000, 1, 3)) * 0.05 + rng.normal(size=(4000, 3, 3)) * 0.004
    return np.concatenate([dense, shell(1000, 12, 0.05) * 3.0])


def _duplicated():
    return np.repeat(shell(150, 21), 2, axis=0)          # equal keys on every axis: the index decides


def _same_centroid():
    rng = np.random.default_rng(22)
    d = np.round(rng.normal(size=(100, 3, 3)) * 64) / 64  # dyadic offsets, so every sum below is exact
    d[:, 2] = -(d[:, 0] + d[:, 1])                        # the three corners' offsets sum to 0: every centroid is (1, 2, 3)
    return d + np.array([1.0, 2.0, 3.0])


def _flat():
    t = shell(300, 23)
    t[:, :, 1] = 0.0                                      # an extent of 0 in y
    return t


def _signed_zeros():
    t = shell(200, 24)
    t[:100, :, 0] = -0.0                                  # centroid x = (-0.0 + -0.0 + -0.0) / 3 = -0.0
    t[100:, :, 0] = 0.0
    return t


def _huge():
    t = shell(241, 25)
    # its box is 2.6e154 x 1.3e154: dx * dy overflows, so the area of every range that holds it is infinite and no split of one has
    # a finite cost (each corner's own length stays finite, 1.3e154^2 < DBL_MAX: scene creation refuses a vertex whose length is not)
    t[7] = [[-1.3e154, 0.0, 0.5], [1.3e154, 0.0, 0.5], [0.0, 1.3e154, 0.5]]
    return t


def _nan_area():
    """CPU only (scene creation refuses coordinates beyond 1e300): one triangle spans -1e308 .. 1e308 in x, so hi - lo is infinite,
    in a mesh flat in y: dx * dy = inf * 0, a NaN area and NaN costs wherever it is inside"""
    t = shell(241, 26)
    t[:, :, 1] = 0.0
    t[9] = [[-1e308, 0.0, 0.1], [1e308, 0.0, 0.1], [0.0, 0.0, 0.2]]
    return t


MESHES = {
    "n1": lambda: shell(1, 1), "n2": lambda: shell(2, 2), "n15": lambda: shell(15, 3), "n16": lambda: shell(16, 4),
    "n17": lambda: shell(17, 5), "n31": lambda: shell(31, 6), "n240": lambda: shell(240, 7), "n241": lambda: shell(241, 8),
    "n257": lambda: shell(257, 9),
    "duplicated": _duplicated, "same_centroid": _same_centroid, "flat": _flat, "signed_zeros": _signed_zeros, "huge": _huge,
    "uv_sphere": uv_sphere, "n65537": lambda: shell(65537, 10, 0.004), "n300000": lambda: shell(300000, 13, 0.002),
}
CPU_ONLY = {"nan_area": _nan_area}
# the meshes the quality bound is set on
QUALITY = {"uv_sphere": uv_sphere, "shell241": lambda: shell(241, 8), "shell3000": lambda: shell(3000, 14),
           "shell100000": lambda: shell(100000, 15, 0.004), "cluster": cluster}


def geom(tris):
    """(n, 3, 3) corners -> (n, 9) v0, e1, e2 as the scene stores a triangle"""
    tris = np.asarray(tris, dtype=np.float64)
    return np.ascontiguousarray(np.concatenate([tris[:, 0], tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0]], axis=1))


@functools.lru_cache(maxsize=None)
def mesh(name):
    t = (MESHES.get(name) or QUALITY.get(name) or CPU_ONLY[name])()
    t.setflags(write=False)
    return t


def compile_harness(out_dir, extra=(), program=False):
    """g++ build of tests/bvh_sweep_harness.cpp: the shared library, or with program=True the stand-alone program"""
    out = os.path.join(str(out_dir), "sweep_main" if program else "libbvh_sweep.so")
    # -Bsymbolic: the harness calls ITS builders (inline members are weak symbols, and librt_hip.so exports the product's)
    kind = ["-DSWEEP_MAIN"] if program else ["-shared", "-fPIC", "-Wl,-Bsymbolic"]
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off"] + kind + list(extra) +
                   ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "raytracer.c_amd", "csrc"),
                    os.path.join(ROOT, "tests", "bvh_sweep_harness.cpp"), "-o", out], check=True)
    return out


class Sweep:
    """BvhSweep through the harness"""

    def __init__(self, so):
        self.lib = C.CDLL(so)
        self.lib.sweep_check.restype = C.c_int
        self.lib.sweep_check.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32 * 4), C.POINTER(C.c_double)]
        self.lib.sweep_fetch.restype = None
        self.lib.sweep_fetch.argtypes = [C.c_void_p] * 4
        self.lib.host_tree_cost.restype = C.c_double
        self.lib.host_tree_cost.argtypes = [C.c_void_p, C.c_uint32]

    def build(self, g):
        """-> dict(rc, depth, max_depth, n_nodes, leaves, cost, nodes (n_nodes, 16), order, axis, left)"""
        out, cost = (C.c_uint32 * 4)(), C.c_double()
        rc = self.lib.sweep_check(g.ctypes.data, len(g), C.byref(out), C.byref(cost))
        r = dict(rc=rc)
        if rc == 0:
            nn = out[2]
            nodes, order = np.zeros((nn, SRC_DOUBLES)), np.zeros(len(g), dtype=np.uint32)
            ns = nn if len(g) > LEAF else 0
            axis, left = np.zeros(ns, dtype=np.uint32), np.zeros(ns, dtype=np.uint32)
            self.lib.sweep_fetch(nodes.ctypes.data, order.ctypes.data, axis.ctypes.data if ns else None, left.ctypes.data if ns else None)
            r.update(depth=out[0], max_depth=out[1], n_nodes=nn, leaves=out[3], cost=cost.value, nodes=nodes, order=order, axis=axis,
                     left=left)
        return r

    def host_cost(self, g):
        return self.lib.host_tree_cost(g.ctypes.data, len(g))


def node_refs(nodes):
    """(n_nodes, 2) uint32: the two child refs of every node"""
    return np.ascontiguousarray(nodes[:, 12]).view(np.uint32).reshape(-1, 2)


def node_ranges(nodes):
    """[b, e) of every node in the leaf order, from the refs alone"""
    refs = node_refs(nodes)
    rng = np.zeros((len(nodes), 2), dtype=np.int64)
    child = np.zeros((len(nodes), 2, 2), dtype=np.int64)
    for k in range(len(nodes) - 1, -1, -1):       # breadth-first numbering: children come after their parent
        for c in range(2):
            r = int(refs[k, c])
            if r & LEAF_FLAG:
                b = (r & ~LEAF_FLAG) >> COUNT_BITS
                child[k, c] = (b, b + (r & ((1 << COUNT_BITS) - 1)))
            else:
                assert r > k, "a child's node number must exceed its parent's"
                child[k, c] = rng[r]
        rng[k] = (child[k, 0, 0], child[k, 1, 1])
    return rng, child

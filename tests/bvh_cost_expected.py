"""What the tests of the device cost and of the in-place rebuild share (tests/test_bvh_rebuild_cpu.py, tests/test_gpu_bvh_rebuild.py):
the contract of rt_hip_scene_bvh_cost (include/rt_hip.h) restated twice -- in numpy, and as a scalar Python loop that pins the numpy
text --, the synthetic node arrays at the reduction's edges, the totality cases, and the two committed pairs of position sets whose
device-built trees differ in node count.  Nodes are (n, 16) float64 arrays as rt_hip_scene_bvh_read returns them: two child boxes
(lo xyz, hi xyz each), the two uint32 refs in the bytes of column 12, padding."""
import numpy as np

import bvh_sweep_meshes as M

BLOCK = 256                      # BVH_COST_BLOCK
COUNT_MASK = (1 << M.COUNT_BITS) - 1
EDGE_SIZES = (1, 2, 255, 256, 257, 65535, 65536, 65537)   # the block edges and the edges of the second and third level
SEED = 20261020


def refs_of(nodes):
    return np.ascontiguousarray(nodes[:, 12]).view(np.uint32).reshape(-1, 2)


def pack_refs(nodes, refs):
    nodes[:, 12] = np.ascontiguousarray(refs, dtype=np.uint32).reshape(-1, 2).view(np.float64)[:, 0]


# ---- the restatement in numpy ----
def _half_area(lo, hi):
    d = hi - lo
    return d[..., 0] * d[..., 1] + d[..., 1] * d[..., 2] + d[..., 2] * d[..., 0]


def root_area(nodes):
    n0 = nodes[0]
    with np.errstate(all="ignore"):
        return float(_half_area(np.fmin(n0[0:3], n0[6:9]), np.fmax(n0[3:6], n0[9:12])))


def terms(nodes, a_root):
    """(n,) the nodes' terms (c0 + c1)"""
    refs = refs_of(nodes)
    c = []
    with np.errstate(all="ignore"):
        for k in range(2):
            leaf = (refs[:, k] & M.LEAF_FLAG) != 0
            count = (refs[:, k] & COUNT_MASK).astype(np.float64)
            box = nodes[:, 6 * k:6 * k + 6]
            v = (_half_area(box[:, 0:3], box[:, 3:6]) / a_root) * np.where(leaf, 45.0 * count, 60.0)
            c.append(np.where(leaf & (count == 0), 0.0, v))
        return c[0] + c[1]


def tree_sum(v):
    """the fixed tree: blocks of 256 (missing terms +0.0), v[i] = v[i] + v[i + m] for m = 128 .. 1; the block sums likewise"""
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(all="ignore"):
        while True:
            nb = -(-len(v) // BLOCK)
            b = np.zeros(nb * BLOCK)
            b[:len(v)] = v
            b = b.reshape(nb, BLOCK)
            m = BLOCK // 2
            while m >= 1:
                b = b[:, :m] + b[:, m:2 * m]
                m //= 2
            v = b[:, 0]
            if nb == 1:
                return float(v[0])


def cost(nodes):
    nodes = np.ascontiguousarray(nodes, dtype=np.float64).reshape(-1, M.SRC_DOUBLES)
    if len(nodes) == 0:
        return 0.0
    a = root_area(nodes)
    if not (a > 0) or not (a < 1e300):
        return 0.0
    return 60.0 + tree_sum(terms(nodes, a))


# ---- the same contract as a scalar loop over Python floats (IEEE doubles, one rounding an operation) ----
def _fmin(a, b):
    return b if a != a else a if b != b else min(a, b)


def _fmax(a, b):
    return b if a != a else a if b != b else max(a, b)


def _half_area_s(lo, hi):
    dx, dy, dz = hi[0] - lo[0], hi[1] - lo[1], hi[2] - lo[2]
    return dx * dy + dy * dz + dz * dx


def _div(a, b):
    return float(np.float64(a) / np.float64(b))       # IEEE division: Python raises where b is 0


def cost_scalar(nodes):
    nodes = np.ascontiguousarray(nodes, dtype=np.float64).reshape(-1, M.SRC_DOUBLES)
    if len(nodes) == 0:
        return 0.0
    refs = refs_of(nodes).tolist()
    rows = nodes.tolist()
    n0 = rows[0]
    a_root = _half_area_s([_fmin(n0[k], n0[6 + k]) for k in range(3)], [_fmax(n0[3 + k], n0[9 + k]) for k in range(3)])
    if not (a_root > 0) or not (a_root < 1e300):
        return 0.0
    v = []
    with np.errstate(all="ignore"):
        for n, r in zip(rows, refs):
            c = []
            for k in range(2):
                leaf, count = (r[k] & M.LEAF_FLAG) != 0, r[k] & COUNT_MASK
                if leaf and count == 0:
                    c.append(0.0)
                else:
                    c.append(_div(_half_area_s(n[6 * k:6 * k + 3], n[6 * k + 3:6 * k + 6]), a_root) * (45.0 * count if leaf else 60.0))
            v.append(c[0] + c[1])
    while True:
        sums = []
        for first in range(0, len(v), BLOCK):
            b = v[first:first + BLOCK] + [0.0] * (BLOCK - len(v[first:first + BLOCK]))
            m = BLOCK // 2
            while m >= 1:
                for i in range(m):
                    b[i] = b[i] + b[i + m]
                m //= 2
            sums.append(b[0])
        v = sums
        if len(v) == 1:
            return 60.0 + v[0]


def same_cost(a, b):
    """bit for bit; a NaN equals a NaN (its sign and payload are not part of the contract)"""
    a, b = np.float64(a), np.float64(b)
    return bool(a.view(np.uint64) == b.view(np.uint64) or (np.isnan(a) and np.isnan(b)))


# ---- synthetic nodes: no tree, only bytes of the kinds a tree holds (no ref is followed by the contract) ----
def synthetic_nodes(n, seed=SEED):
    """n nodes: node 0's boxes inside [-8, 8]^3 and wide, the others' boxes anywhere inside with sizes over six decades; refs a mix
    of inner refs, leaves of 1..15 and empty leaves; padding left 0"""
    rng = np.random.default_rng([seed, n])
    nodes = np.zeros((n, M.SRC_DOUBLES))
    lo = rng.uniform(-8.0, 7.0, size=(n, 2, 3))
    size = 10.0 ** rng.uniform(-5.0, 0.0, size=(n, 2, 3))
    nodes[:, :12] = np.concatenate([lo, lo + size], axis=2).reshape(n, 12)
    nodes[0, :12] = [-8, -8, -8, 1, 2, 3, -2, -1, -3, 8, 8, 8]
    kind = rng.integers(0, 8, size=(n, 2))
    refs = np.where(kind < 3, rng.integers(0, 1 << 27, size=(n, 2)),
                    M.LEAF_FLAG | (rng.integers(0, 1 << 20, size=(n, 2)) << M.COUNT_BITS) | rng.integers(1, 16, size=(n, 2)))
    refs = np.where(kind == 7, M.LEAF_FLAG | (rng.integers(0, 1 << 20, size=(n, 2)) << M.COUNT_BITS), refs)
    pack_refs(nodes, refs.astype(np.uint32))
    return nodes


def totality_cases():
    """name -> nodes: what no builder makes, and a defined result all the same"""
    base = synthetic_nodes(300, SEED + 1)
    out = {}

    def case(name, edit):
        a = base.copy()
        edit(a)
        out[name] = a

    case("nan_child_box", lambda a: a.__setitem__((17, 2), np.nan))                       # a NaN term: the cost is NaN
    case("nan_in_one_root_box", lambda a: a.__setitem__((0, slice(0, 6)), np.nan))        # fmin / fmax take the other box
    case("nan_root", lambda a: a.__setitem__((0, slice(0, 12)), np.nan))                  # no area: 0.0
    case("inf_root", lambda a: a.__setitem__((0, 3), np.inf))                             # an area that is not < 1e300: 0.0
    case("huge_root", lambda a: a.__setitem__((0, slice(9, 12)), 1e151))                  # 3e302: 0.0
    case("inf_child_box", lambda a: a.__setitem__((200, 9), np.inf))                      # an infinite term
    case("inf_minus_inf", lambda a: (a.__setitem__((5, 3), np.inf), a.__setitem__((260, 0), np.inf)))  # +inf and -inf terms meet
    case("inverted_child_box", lambda a: a.__setitem__((40, slice(0, 6)), [1, 1, 1, 0, 0.5, -2]))
    case("zero_area_root", lambda a: a.__setitem__((0, slice(0, 12)), [1, 2, 3, 1, 2, 3] * 2))
    case("flat_root", lambda a: a.__setitem__((0, slice(0, 12)), [0, 0, 0, 4, 0, 0] * 2))  # two extents of 0: area 0
    case("inverted_root", lambda a: a.__setitem__((0, slice(0, 12)), [1, 1, 1, 0, 0, 2] * 2))   # a negative area: 0.0
    case("garbage_refs", lambda a: pack_refs(a, np.random.default_rng(SEED + 2).integers(0, 1 << 32, size=(len(a), 2), dtype=np.uint64)
                                              .astype(np.uint32)))
    case("padding_ignored", lambda a: a.__setitem__((slice(None), slice(13, 16)), np.nan))
    one = np.zeros((1, M.SRC_DOUBLES))      # a one-leaf root as both builders make it: the leaf's box twice, an empty second child
    one[0, :12] = [-1, -2, -3, 1, 2, 3] * 2
    pack_refs(one, np.array([[M.LEAF_FLAG | 7, M.LEAF_FLAG]], dtype=np.uint32))
    out["one_leaf_root"] = one
    return out


# ---- two pairs of position sets of equal triangle count whose device-built trees differ in node count ----
# (n, seed of the first set, seed of the second): M.shell(n, seed) * 3.  tests/test_bvh_rebuild_cpu.py asserts the inequality with
# BvhSweep, so tests/test_gpu_bvh_rebuild.py, which moves a scene from the first set to the second and back, crosses the node
# capacity in the direction the name says at its first rebuild.
PAIRS = {"grows": (300, 104, 103), "shrinks": (241, 100, 102)}      # 25 -> 30 nodes; 23 -> 20 nodes


# one scene taken through position sets whose trees have ever more nodes (25 < 28 < 30): the second rebuild needs a side
# allocation larger than the one the first made
CLIMB = (300, (104, 101, 103))


def climb():
    n, seeds = CLIMB
    return [np.array(M.shell(n, s)) * 3.0 for s in seeds]


def pair(name):
    n, s0, s1 = PAIRS[name]
    return np.array(M.shell(n, s0)) * 3.0, np.array(M.shell(n, s1)) * 3.0

// CPU check of BvhSweep (raytracer.c_amd/csrc/bvh_build.h), the sequential statement of the tree the device builder makes:
// compiled by g++ -ffp-contract=off in tests/test_bvh_sweep_cpu.py (a shared library the tests call), and once more with
// -DSWEEP_MAIN -fsanitize=address,undefined as a stand-alone program.  sweep_check() builds the tree over n triangles (9 doubles
// each: v0, e1, e2), keeps it for sweep_fetch(), and returns 0 when the invariants tests/bvh_harness.cpp asks of the host tree hold:
//   11 order is a permutation;  20-22 the leaves tile [0, n) left to right, each 0 < count <= PT_BVH_LEAF (an empty second child
//   only at the root of a one-leaf mesh), refs stay inside the node array;  12 max_depth is the least depth such leaves allow and
//   depth <= it;  23 every stored child box is, bit for bit, the min / max of its members' boxes;  13 the counts add up and depth
//   is the longest path;  10 two builds agree;  14 the per-node splits on record are one per node.
// out[0] = depth, out[1] = max_depth, out[2] = nodes, out[3] = leaves; *cost = tree_cost().
#include <cstdio>
#include "bvh_build.h"

namespace
{
BvhSweep g_kept;

struct Walk
{
  const BvhSweep &b;
  uint32_t next_first = 0, leaves = 0;
  int longest = 0, err = 0;
  uint32_t visit(uint32_t ref, double *box, int level, bool root_child1)
  {
    for (int k = 0; k < 3; k++)
    {
      box[k] = HUGE_VAL;
      box[3 + k] = -HUGE_VAL;
    }
    if (ref & PT_BVH_LEAF_FLAG)
    {
      const uint32_t first = (ref & ~PT_BVH_LEAF_FLAG) >> PT_BVH_COUNT_BITS, count = ref & ((1u << PT_BVH_COUNT_BITS) - 1u);
      if (count == 0)
      {
        if (!root_child1)
          err = err ? err : 20;
        return 0;
      }
      if (count > PT_BVH_LEAF || first != next_first || (size_t)first + count > b.order.size())
      {
        err = err ? err : 21;
        return 0;
      }
      next_first = first + count;
      leaves++;
      for (uint32_t i = first; i < first + count; i++)
        for (int k = 0; k < 3; k++)
        {
          box[k] = bvh_min(box[k], b.box[6 * (size_t)b.order[i] + k]);
          box[3 + k] = bvh_max(box[3 + k], b.box[6 * (size_t)b.order[i] + 3 + k]);
        }
      return count;
    }
    if ((size_t)ref * PT_BVH_SRC_DOUBLES >= b.nodes.size() || level > 64)
    {
      err = err ? err : 22;
      return 0;
    }
    longest = std::max(longest, level + 1);
    const double *n = &b.nodes[(size_t)ref * PT_BVH_SRC_DOUBLES];
    uint32_t refs[2];
    memcpy(refs, n + 12, sizeof refs);
    uint32_t total = 0;
    for (int c = 0; c < 2; c++)
    {
      double cb[6];
      const uint32_t cnt = visit(refs[c], cb, level + 1, level == 0 && c == 1 && b.nodes.size() == PT_BVH_SRC_DOUBLES);
      if (cnt != 0 && memcmp(cb, n + 6 * c, sizeof cb) != 0)
        err = err ? err : 23;
      for (int k = 0; k < 3; k++)
      {
        box[k] = bvh_min(box[k], cb[k]);
        box[3 + k] = bvh_max(box[3 + k], cb[3 + k]);
      }
      total += cnt;
    }
    return total;
  }
};
} // namespace

extern "C" int sweep_check(const double *tgeom, uint32_t n, uint32_t out[4], double *cost)
{
  if (n == 0)
    return 1;
  BvhSweep &a = g_kept;
  BvhSweep again;
  a.tgeom = again.tgeom = tgeom;
  a.build_root(n);
  again.build_root(n);
  if (a.order != again.order || a.depth != again.depth || a.nodes.size() != again.nodes.size() ||
      memcmp(a.nodes.data(), again.nodes.data(), a.nodes.size() * sizeof(double)) != 0)
    return 10;
  if (a.order.size() != n)
    return 11;
  std::vector<uint8_t> seen(n, 0);
  for (uint32_t t : a.order)
  {
    if (t >= n || seen[t])
      return 11;
    seen[t] = 1;
  }
  int least = 0;
  while (((uint64_t)PT_BVH_LEAF << least) < n)
    least++;
  if (a.max_depth != least || a.depth > std::max(least, 1))
    return 12;
  Walk w{a};
  double box[6];
  const uint32_t total = w.visit(0u, box, 0, false);
  if (w.err)
    return w.err;
  if (total != n || w.next_first != n || w.longest != a.depth)
    return 13;
  const size_t n_nodes = a.nodes.size() / PT_BVH_SRC_DOUBLES;
  if (n > PT_BVH_LEAF && (a.split_axis.size() != n_nodes || a.split_left.size() != n_nodes))
    return 14;
  out[0] = (uint32_t)a.depth;
  out[1] = (uint32_t)a.max_depth;
  out[2] = (uint32_t)n_nodes;
  out[3] = w.leaves;
  *cost = a.tree_cost();
  return 0;
}

// the tree sweep_check() built last: nodes (out[2] x PT_BVH_SRC_DOUBLES), order (n), and per node the split's axis and left count
// (meshes above one leaf); any pointer may be null
extern "C" void sweep_fetch(double *nodes, uint32_t *order, uint32_t *split_axis, uint32_t *split_left)
{
  const BvhSweep &a = g_kept;
  if (nodes)
    memcpy(nodes, a.nodes.data(), a.nodes.size() * sizeof(double));
  if (order)
    memcpy(order, a.order.data(), a.order.size() * sizeof(uint32_t));
  if (split_axis)
    memcpy(split_axis, a.split_axis.data(), a.split_axis.size() * sizeof(uint32_t));
  if (split_left)
    memcpy(split_left, a.split_left.data(), a.split_left.size() * sizeof(uint32_t));
}

// tree_cost() of the host builder's tree (BvhBuild::build_root) over the same triangles: what the quality bound is against
extern "C" double host_tree_cost(const double *tgeom, uint32_t n)
{
  BvhBuild b;
  b.tgeom = tgeom;
  b.order.resize(n);
  b.cen.resize(3 * (size_t)n);
  b.lo.resize(3 * (size_t)n);
  b.hi.resize(3 * (size_t)n);
  for (uint32_t k = 0; k < n; k++)
  {
    b.order[k] = k;
    b.tri_box(k);
  }
  b.build_root(n);
  return b.tree_cost();
}

#ifdef SWEEP_MAIN
// stand-alone (the sanitizer build): triangles from stdin-free generators of its own, the sizes where a mechanism changes
static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static double rnd()
{
  g_rng ^= g_rng << 13;
  g_rng ^= g_rng >> 7;
  g_rng ^= g_rng << 17;
  return (double)(g_rng >> 11) / 9007199254740992.0 - 0.5;
}

int main()
{
  const uint32_t sizes[] = {1, 2, 15, 16, 17, 31, 240, 241, 257, 3000, 20000};
  int bad = 0;
  for (int variant = 0; variant < 5; variant++)
    for (uint32_t n : sizes)
    {
      if (variant != 0 && n > 3000)
        continue;
      std::vector<double> g(9 * (size_t)n);
      for (uint32_t t = 0; t < n; t++)
      {
        if (variant == 1 && (t & 1)) // 1: every triangle twice
        {
          memcpy(&g[9 * (size_t)t], &g[9 * (size_t)(t - 1)], 9 * sizeof(double));
          continue;
        }
        for (int k = 0; k < 3; k++)
        {
          double c = 20.0 * rnd();
          if (variant == 2)
            c = 1.0; // all centroids alike
          if (variant == 3 && k == 1)
            c = 0.0; // flat in y
          g[9 * (size_t)t + k] = c;
          g[9 * (size_t)t + 3 + k] = variant == 3 && k == 1 ? 0.0 : (variant == 2 ? 0.0 : 0.3 * rnd());
          g[9 * (size_t)t + 6 + k] = variant == 3 && k == 1 ? -0.0 : (variant == 2 ? 0.0 : 0.3 * rnd());
        }
        if (variant == 4 && t == 0) // a box of 1e200 x 1e200: dx * dy overflows, every cost of a range that holds it is infinite
          g[3] = g[7] = 1e200;
      }
      uint32_t out[4];
      double cost;
      const int rc = sweep_check(g.data(), n, out, &cost);
      if (rc != 0)
      {
        printf("variant %d n %u: invariant %d\n", variant, n, rc);
        bad = 1;
      }
    }
  printf(bad ? "FAILED\n" : "sweep ok\n");
  return bad;
}
#endif

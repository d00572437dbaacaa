// CPU check of BvhRefit (raytracer.c_amd/csrc/bvh_build.h), the sequential statement of a refit to moved triangles: compiled by
// g++ -ffp-contract=off in tests/scene_update_meshes.py (a shared library the tests call), and once more with -DREFIT_MAIN
// -fsanitize=address,undefined as a stand-alone program over files of triangles (n x 9 doubles: v0, e1, e2).
//   refit_build(builder, tgeom, n)   builds and keeps a tree: 0 = BvhBuild (the host builder), 1 = BvhSweep (the device's)
//   refit_fetch(nodes, order)        the kept tree
//   refit_apply(nodes, n_nodes, order, tgeom)   BvhRefit::refit in place; 0, or 1 where a child is not numbered above its parent
//   refit_levels(nodes, n_nodes, by_level, level_begin)   BvhRefit::levels; -> the number of levels, 0 on failure
#include <cstdio>
#include "bvh_build.h"

namespace
{
std::vector<double> g_nodes;
std::vector<uint32_t> g_order;
} // namespace

extern "C" uint32_t refit_build(int builder, const double *tgeom, uint32_t n)
{
  if (builder == 1)
  {
    BvhSweep s;
    s.tgeom = tgeom;
    s.build_root(n);
    g_nodes = s.nodes;
    g_order = s.order;
  }
  else
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
    g_nodes = b.nodes;
    g_order = b.order;
  }
  return (uint32_t)(g_nodes.size() / PT_BVH_SRC_DOUBLES);
}

extern "C" void refit_fetch(double *nodes, uint32_t *order)
{
  if (nodes)
    memcpy(nodes, g_nodes.data(), g_nodes.size() * sizeof(double));
  if (order)
    memcpy(order, g_order.data(), g_order.size() * sizeof(uint32_t));
}

extern "C" int refit_apply(double *nodes, uint32_t n_nodes, const uint32_t *order, const double *tgeom)
{
  return BvhRefit::refit(nodes, n_nodes, order, tgeom) ? 0 : 1;
}

extern "C" uint32_t refit_levels(const double *nodes, uint32_t n_nodes, uint32_t *by_level, uint32_t *level_begin)
{
  std::vector<uint32_t> bl, lb;
  if (!BvhRefit::levels(nodes, n_nodes, bl, lb))
    return 0;
  memcpy(by_level, bl.data(), bl.size() * sizeof(uint32_t));
  memcpy(level_begin, lb.data(), lb.size() * sizeof(uint32_t));
  return (uint32_t)(lb.size() - 1);
}

#ifdef REFIT_MAIN
// stand-alone (the sanitizer build): refit_main FILE...  Each file holds n x 9 doubles.  Per file and builder: the identity refit
// keeps every box (bytes for BvhSweep's tree, values for BvhBuild's, whose fmin may have kept the other zero), a deformed mesh's
// refit gives at every child the join of its range's triangle boxes (recomputed here by a walk of its own), refs, padding and the
// empty child untouched, and the levels sort every node once with children one level below their parent.
namespace
{
void walk_box(const std::vector<double> &nodes, const std::vector<uint32_t> &order, const double *tgeom, uint32_t ref, double *box)
{
  BvhRefit::empty(box);
  if (ref & PT_BVH_LEAF_FLAG)
  {
    const uint32_t first = (ref & ~PT_BVH_LEAF_FLAG) >> PT_BVH_COUNT_BITS, count = ref & ((1u << PT_BVH_COUNT_BITS) - 1u);
    for (uint32_t j = 0; j < count; j++)
    {
      double tb[6], cen[3];
      bvh_tri_box(tgeom + 9 * (size_t)order[first + j], tb, cen);
      BvhRefit::join(box, tb);
    }
    return;
  }
  for (int c = 0; c < 2; c++)
  {
    double cb[6];
    walk_box(nodes, order, tgeom, BvhRefit::child_ref(nodes.data(), ref, c), cb);
    BvhRefit::join(box, cb);
  }
}

int check_file(const char *path)
{
  FILE *f = fopen(path, "rb");
  if (!f)
    return 100;
  std::vector<double> g;
  double buf[9];
  while (fread(buf, sizeof(double), 9, f) == 9)
    g.insert(g.end(), buf, buf + 9);
  fclose(f);
  const uint32_t n = (uint32_t)(g.size() / 9);
  if (n == 0)
    return 101;
  std::vector<double> moved(g);
  for (uint32_t t = 0; t < n; t++) // a shear and a scale: v0 moves, the edges stretch
    for (int k = 0; k < 3; k++)
    {
      moved[9 * (size_t)t + k] = 1.3 * g[9 * (size_t)t + k] + 0.25 * g[9 * (size_t)t + (k + 1) % 3] - 0.1;
      moved[9 * (size_t)t + 3 + k] = 1.3 * g[9 * (size_t)t + 3 + k] + 0.25 * g[9 * (size_t)t + 3 + (k + 1) % 3];
      moved[9 * (size_t)t + 6 + k] = 1.3 * g[9 * (size_t)t + 6 + k] + 0.25 * g[9 * (size_t)t + 6 + (k + 1) % 3];
    }
  for (int builder = 0; builder < 2; builder++)
  {
    const uint32_t n_nodes = refit_build(builder, g.data(), n);
    const std::vector<double> before = g_nodes;
    std::vector<double> nodes = g_nodes;
    if (refit_apply(nodes.data(), n_nodes, g_order.data(), g.data()) != 0)
      return 1;
    for (size_t i = 0; i < nodes.size(); i++)
      if (builder == 1 ? memcmp(&nodes[i], &before[i], 8) != 0 : (i % PT_BVH_SRC_DOUBLES < 12 ? !(nodes[i] == before[i]) : memcmp(&nodes[i], &before[i], 8) != 0))
        return 2;
    if (refit_apply(nodes.data(), n_nodes, g_order.data(), moved.data()) != 0)
      return 3;
    for (uint32_t i = 0; i < n_nodes; i++)
    {
      if (memcmp(&nodes[i * (size_t)PT_BVH_SRC_DOUBLES + 12], &before[i * (size_t)PT_BVH_SRC_DOUBLES + 12], 4 * sizeof(double)) != 0)
        return 4;
      for (int c = 0; c < 2; c++)
      {
        const uint32_t ref = BvhRefit::child_ref(nodes.data(), i, c);
        const double *have = &nodes[i * (size_t)PT_BVH_SRC_DOUBLES + 6 * c];
        if (BvhRefit::is_leaf(ref) && BvhRefit::leaf_count(ref) == 0)
        {
          if (memcmp(have, &before[i * (size_t)PT_BVH_SRC_DOUBLES + 6 * c], 6 * sizeof(double)) != 0)
            return 5;
          continue;
        }
        double want[6];
        walk_box(nodes, g_order, moved.data(), ref, want);
        if (memcmp(have, want, sizeof want) != 0)
          return 6;
      }
    }
    std::vector<uint32_t> by_level(n_nodes), level_begin(n_nodes + 2), depth(n_nodes, 0);
    const uint32_t n_levels = refit_levels(nodes.data(), n_nodes, by_level.data(), level_begin.data());
    if (n_levels == 0 || level_begin[0] != 0 || level_begin[n_levels] != n_nodes)
      return 7;
    std::vector<uint8_t> seen(n_nodes, 0);
    for (uint32_t d = 0; d < n_levels; d++)
      for (uint32_t k = level_begin[d]; k < level_begin[d + 1]; k++)
      {
        if (by_level[k] >= n_nodes || seen[by_level[k]])
          return 8;
        seen[by_level[k]] = 1;
        depth[by_level[k]] = d;
      }
    for (uint32_t i = 0; i < n_nodes; i++)
      for (int c = 0; c < 2; c++)
      {
        const uint32_t ref = BvhRefit::child_ref(nodes.data(), i, c);
        if (!BvhRefit::is_leaf(ref) && depth[ref] != depth[i] + 1)
          return 9;
      }
  }
  return 0;
}
} // namespace

int main(int argc, char **argv)
{
  int bad = 0;
  for (int k = 1; k < argc; k++)
  {
    const int rc = check_file(argv[k]);
    if (rc != 0)
    {
      printf("%s: check %d\n", argv[k], rc);
      bad = 1;
    }
  }
  printf(bad || argc < 2 ? "FAILED\n" : "refit ok\n");
  return bad || argc < 2;
}
#endif

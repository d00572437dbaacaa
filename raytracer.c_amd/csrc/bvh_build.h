/* bvh_build.h -- the host-side builder of the triangle hierarchy (rt_hip_scene_create, rt_hip_shim.hip).
 * Plain C++ (no HIP): also compiled by g++ into the CPU test of its invariants (tests/bvh_harness.cpp, tests/test_host.py).
 * Below it BvhSweep, the sequential statement of the tree the device builder makes (tests/bvh_sweep_harness.cpp), BvhRefit, the
 * statement of a refit to moved triangles (tests/bvh_refit_harness.cpp), and -- for HIP translation units only -- the device
 * builder's interface (bvh_device.hip). */
#ifndef BVH_BUILD_H
#define BVH_BUILD_H

#include <algorithm>
#include <cassert>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pt_device.h"

/* ---- bounding-volume hierarchy over triangles ----
 * Binary tree, leaves of <= PT_BVH_LEAF triangles, of the LEAST depth such leaves allow (max_depth = the smallest D with
 * PT_BVH_LEAF * 2^D >= n: a lane's traversal stack in LDS is sized by the depth, and one level more costs config 5's kernel its
 * fourth workgroup per CU).  Within that depth a node is split by the surface-area heuristic over 64 bins of the centroid
 * bounds on each axis (round 4; cost = area(left box) * count(left) + area(right box) * count(right), only splits that leave
 * both sides a subtree of the remaining depth: count <= PT_BVH_LEAF * 2^(levels left)); where no such split exists -- or with
 * RT_HIP_BVH_MEDIAN=1, round 1-3's builder, for A/B -- by the median on the longest axis of the centroid bounds, which always
 * does.  On config 5's 10,240-triangle sphere: node visits per walked ray 15.3 -> 13.9, leaf pre-tests 21.0 -> 18.3, leaves
 * 2.1 -> 1.6 at the same depth of 10.  A node stores the boxes of its two
 * children, so the device tests both with one set of packed-fp32 instructions, descends into
 * the nearer one first and keeps the other on a small per-lane stack (bvh_traverse).  The
 * hierarchy only decides WHICH triangles get the exact test; the exact test and the
 * (t, index) tie rule decide the result, so any valid hierarchy gives the linear scan's answer. */
struct BvhBuild
{
  const double *tgeom;              /* n_tri x 9: v0, e1, e2 */
  std::vector<uint32_t> order;      /* triangle indices, permuted in place */
  std::vector<double> nodes;        /* PT_BVH_SRC_DOUBLES per node: the two children's boxes + refs */
  std::vector<double> cen, lo, hi;  /* per triangle: centroid, box */
  std::vector<uint8_t> bin_of;      /* per triangle: its bin on the axis being tried (scratch of the split search) */
  int depth = 0;                    /* inner nodes on the longest root-to-leaf path */
  int max_depth = 0;                /* the least depth leaves of PT_BVH_LEAF allow: no split may exceed it */
  bool median_only = false;         /* the tree being built splits at the median everywhere */
  bool used_area_splits = false;    /* build_root kept the surface-area tree (it was the cheaper one by tree_cost) */

  static double half_area(const double *l, const double *h)
  {
    const double dx = h[0] - l[0], dy = h[1] - l[1], dz = h[2] - l[2];
    return dx * dy + dy * dz + dz * dx;
  }

  /* The surface-area split of order[begin, end) on the bins of the centroid bounds [cl, ch]: partitions the range (stably, so the
   * build is deterministic) and returns the size of its left part, or 0 when no admissible split exists.  `cap` = the most
   * triangles a side may hold and still fit a subtree of the remaining depth. */
  uint32_t sah_split(uint32_t begin, uint32_t end, const double *cl, const double *ch, uint64_t cap)
  {
    constexpr int NB = 64;
    const uint32_t n = end - begin;
    double best = 1e300;
    int best_axis = -1, best_split = 0;
    uint32_t best_left = 0;
    for (int axis = 0; axis < 3; axis++)
    {
      const double ext = ch[axis] - cl[axis];
      if (!(ext > 0) || !(ext < 1e300))
        continue;
      const double scale = NB / ext;
      uint32_t cnt[NB] = {0};
      double blo[NB][3], bhi[NB][3];
      for (int b = 0; b < NB; b++)
        for (int k = 0; k < 3; k++)
        {
          blo[b][k] = 1e300;
          bhi[b][k] = -1e300;
        }
      for (uint32_t i = begin; i < end; i++)
      {
        const uint32_t t = order[i];
        const int b = std::min(NB - 1, std::max(0, (int)((cen[3 * t + axis] - cl[axis]) * scale)));
        cnt[b]++;
        for (int k = 0; k < 3; k++)
        {
          blo[b][k] = std::fmin(blo[b][k], lo[3 * t + k]);
          bhi[b][k] = std::fmax(bhi[b][k], hi[3 * t + k]);
        }
      }
      /* right-hand boxes and counts by a sweep from the top, then the left-hand ones with the candidate splits */
      double r_area[NB];
      uint32_t r_cnt[NB];
      {
        double l3[3] = {1e300, 1e300, 1e300}, h3[3] = {-1e300, -1e300, -1e300};
        uint32_t c = 0;
        for (int b = NB - 1; b >= 1; b--)
        {
          for (int k = 0; k < 3; k++)
          {
            l3[k] = std::fmin(l3[k], blo[b][k]);
            h3[k] = std::fmax(h3[k], bhi[b][k]);
          }
          c += cnt[b];
          r_cnt[b] = c;
          r_area[b] = c ? half_area(l3, h3) : 0.0;
        }
      }
      double l3[3] = {1e300, 1e300, 1e300}, h3[3] = {-1e300, -1e300, -1e300};
      uint32_t c = 0;
      for (int sp = 1; sp < NB; sp++) /* bins [0, sp) go left */
      {
        for (int k = 0; k < 3; k++)
        {
          l3[k] = std::fmin(l3[k], blo[sp - 1][k]);
          h3[k] = std::fmax(h3[k], bhi[sp - 1][k]);
        }
        c += cnt[sp - 1];
        if (c == 0 || c == n || c > cap || r_cnt[sp] > cap)
          continue;
        const double cost = half_area(l3, h3) * c + r_area[sp] * r_cnt[sp];
        if (cost < best)
        {
          best = cost;
          best_axis = axis;
          best_split = sp;
          best_left = c;
        }
      }
    }
    if (best_axis < 0)
      return 0;
    const double scale = NB / (ch[best_axis] - cl[best_axis]);
    for (uint32_t i = begin; i < end; i++)
    {
      const uint32_t t = order[i];
      bin_of[t] = (uint8_t)std::min(NB - 1, std::max(0, (int)((cen[3 * t + best_axis] - cl[best_axis]) * scale)));
    }
    std::stable_partition(order.begin() + begin, order.begin() + end, [&](uint32_t t) { return bin_of[t] < best_split; });
    return best_left;
  }

  void tri_box(uint32_t t)
  {
    const double *g = tgeom + 9 * (size_t)t;
    for (int k = 0; k < 3; k++)
    {
      const double a = g[k], b = g[k] + g[3 + k], c = g[k] + g[6 + k]; /* v0, v0+e1, v0+e2 */
      /* v1 = v0 + e1 is re-rounded here; the slack is absorbed by the device-side margins,
       * which are orders of magnitude larger than one ulp of a coordinate */
      lo[3 * t + k] = std::fmin(a, std::fmin(b, c));
      hi[3 * t + k] = std::fmax(a, std::fmax(b, c));
      cen[3 * t + k] = (a + b + c) / 3.0;
    }
  }

  /* Builds the subtree over order[begin, end) and returns its reference (a leaf reference or
   * the index of its inner node); box[0..5] receives its bounds. */
  uint32_t build(uint32_t begin, uint32_t end, double *box, int level)
  {
    double cl[3] = {1e300, 1e300, 1e300}, ch[3] = {-1e300, -1e300, -1e300};
    for (int k = 0; k < 3; k++)
    {
      box[k] = 1e300;
      box[3 + k] = -1e300;
    }
    for (uint32_t i = begin; i < end; i++)
      for (int k = 0; k < 3; k++)
      {
        const uint32_t t = order[i];
        box[k] = std::fmin(box[k], lo[3 * t + k]);
        box[3 + k] = std::fmax(box[3 + k], hi[3 * t + k]);
        cl[k] = std::fmin(cl[k], cen[3 * t + k]);
        ch[k] = std::fmax(ch[k], cen[3 * t + k]);
      }
    if (end - begin <= PT_BVH_LEAF)
      return PT_BVH_LEAF_FLAG | (begin << PT_BVH_COUNT_BITS) | (end - begin);
    const uint32_t me = (uint32_t)(nodes.size() / PT_BVH_SRC_DOUBLES);
    nodes.resize(nodes.size() + PT_BVH_SRC_DOUBLES, 0.0);
    depth = std::max(depth, level + 1);
    /* either side must fit a subtree of the levels left below this node (the median always does: n <= 2 cap here) */
    const int left_levels = max_depth - level - 1;
    const uint64_t cap = left_levels >= 0 && left_levels < 40 ? ((uint64_t)PT_BVH_LEAF << left_levels) : (uint64_t)PT_BVH_LEAF;
    uint32_t mid = median_only ? 0u : sah_split(begin, end, cl, ch, cap);
    if (mid != 0u)
      mid += begin;
    else
    {
      int axis = 0;
      if (ch[1] - cl[1] > ch[axis] - cl[axis]) axis = 1;
      if (ch[2] - cl[2] > ch[axis] - cl[axis]) axis = 2;
      mid = begin + (end - begin) / 2;
      std::nth_element(order.begin() + begin, order.begin() + mid, order.begin() + end,
                       [&](uint32_t a, uint32_t b) { return cen[3 * a + axis] < cen[3 * b + axis]; });
    }
    double b0[6], b1[6];
    const uint32_t refs[2] = {build(begin, mid, b0, level + 1), build(mid, end, b1, level + 1)};
    double *n = &nodes[PT_BVH_SRC_DOUBLES * (size_t)me]; /* after the recursion: nodes may have moved */
    memcpy(n, b0, sizeof b0);
    memcpy(n + 6, b1, sizeof b1);
    memcpy(n + 12, refs, sizeof refs);
    return me;
  }

  /* What a walk of this tree costs on average, per ray that meets the root's box, in the walk's own instruction counts: a
   * visited inner node tests its two children's boxes (~60 VALU instructions, bvh_test_children), a visited leaf puts its
   * triangles through the fp32 pre-test (~45 each); a box is visited in proportion to its surface area (the usual
   * assumption behind the heuristic).  tools/bvh_sim.py and the device's PT_DIAG counts agree with its ranking on config 5. */
  double tree_cost() const
  {
    if (nodes.empty())
      return 0.0;
    double root[6];
    const double *n0 = &nodes[0];
    for (int k = 0; k < 3; k++)
    {
      root[k] = std::fmin(n0[k], n0[6 + k]);
      root[3 + k] = std::fmax(n0[3 + k], n0[9 + k]);
    }
    const double a_root = half_area(root, root + 3);
    if (!(a_root > 0) || !(a_root < 1e300))
      return 0.0;
    double cost = 60.0; /* the root's own visit */
    for (size_t i = 0; i < nodes.size() / PT_BVH_SRC_DOUBLES; i++)
    {
      const double *n = &nodes[i * PT_BVH_SRC_DOUBLES];
      uint32_t refs[2];
      memcpy(refs, n + 12, sizeof refs);
      for (int c = 0; c < 2; c++)
      {
        const uint32_t count = refs[c] & ((1u << PT_BVH_COUNT_BITS) - 1u);
        if ((refs[c] & PT_BVH_LEAF_FLAG) && count == 0)
          continue; /* the empty second child of a one-leaf mesh */
        const double p = half_area(n + 6 * c, n + 6 * c + 3) / a_root;
        cost += p * ((refs[c] & PT_BVH_LEAF_FLAG) ? 45.0 * count : 60.0);
      }
    }
    return cost;
  }

  void build_tree(uint32_t n_tri)
  {
    double box[6];
    nodes.clear();
    depth = 0;
    const uint32_t ref = build(0, n_tri, box, 0);
    if (ref & PT_BVH_LEAF_FLAG)
    { /* a mesh that fits one leaf still gets a root node: child 0 = the leaf, child 1 = an empty leaf */
      nodes.assign(PT_BVH_SRC_DOUBLES, 0.0);
      const uint32_t refs[2] = {ref, PT_BVH_LEAF_FLAG};
      memcpy(&nodes[0], box, sizeof box);
      memcpy(&nodes[6], box, sizeof box);
      memcpy(&nodes[12], refs, sizeof refs);
      depth = 1;
    }
  }

  /* The whole mesh (order = the caller's initial order, normally the identity).  Both trees are built -- the area splits are
   * greedy, and under the depth cap a lopsided split near the root can use up the slack (PT_BVH_LEAF * 2^max_depth - n) that
   * the levels below would have needed: on a mesh with one dense cluster and little slack the capped area tree came out 20 %
   * dearer than the median tree -- and the one with the lower tree_cost() is kept, so the area heuristic can only help. */
  void build_root(uint32_t n_tri)
  {
    max_depth = 0;
    while (((uint64_t)PT_BVH_LEAF << max_depth) < n_tri)
      max_depth++;
#ifdef PT_DEV_KERNELS
    const char *e = getenv("RT_HIP_BVH_MEDIAN"); /* development builds (A/B, and the two-builders-one-frame test): round 1-3's median builder alone */
    const bool median_asked = e && e[0] == '1';
#else
    const bool median_asked = false;
#endif
    bin_of.assign(n_tri, 0);
    const std::vector<uint32_t> order0 = order;
    median_only = true;
    build_tree(n_tri);
    used_area_splits = false;
    if (median_asked)
      return;
    const double cost_median = tree_cost();
    std::vector<uint32_t> order_m = order;
    std::vector<double> nodes_m = nodes;
    const int depth_m = depth;
    order = order0;
    median_only = false;
    build_tree(n_tri);
    if (tree_cost() < cost_median)
    {
      used_area_splits = true;
      return;
    }
    order.swap(order_m);
    nodes.swap(nodes_m);
    depth = depth_m;
  }
};

/* ---- the device builder's contract: capped full-sweep SAH over three per-axis sorted lists ----
 * bvh_device.hip builds this tree with sorts, segmented scans, a segmented arg-min and stable partitions, level by level; BvhSweep
 * states the same tree in plain sequential C++, and the device's nodes and order are tested against it byte for byte
 * (tests/bvh_sweep_harness.cpp, tests/test_gpu_bvh_device.py).  The pieces both sides must evaluate alike -- the box of a
 * triangle, the sort key, the joins of boxes, the area -- are the functions below, compiled into both (-ffp-contract=off).
 *   per triangle   lo, hi, cen: tri_box's expressions; min / max break the tie of -0.0 and 0.0 (-0.0 is the smaller), so a box
 *                  does not depend on the order its members were joined in (fmin / fmax leave that to the implementation)
 *   lists          L0, L1, L2: all triangle indices, La ascending by (cen[a] + 0.0, index)
 *   levels         level l holds ranges [b, e), each the same set of triangles in all three lists; <= PT_BVH_LEAF: a leaf
 *   split search   m = e - b, cap = PT_BVH_LEAF << (max_depth - l - 1); for a = 0, 1, 2 and i = 1 .. m-1 ascending with
 *                  i <= cap && m - i <= cap:  cost = half_area(box La[b, b+i)) * i + half_area(box La[b+i, e)) * (m - i);
 *                  the winner starts as (axis 0, m / 2) at +infinity and is replaced by a strictly smaller cost only
 *   partition      the winner list's first i entries go left; all three lists are partitioned stably by side
 *   nodes          numbered breadth-first (level by level, left to right, root = 0: the walks follow refs only, no kernel
 *                  relies on the host builder's depth-first numbering); order = the final L0; a one-leaf mesh gets the root
 *                  with an empty second leaf; depth = the levels that hold an inner node */
#if defined(__HIPCC__)
#define BVH_HD __host__ __device__
#else
#define BVH_HD
#endif

BVH_HD inline double bvh_min(double a, double b) { return (a < b || (a == b && std::signbit(a))) ? a : b; }
BVH_HD inline double bvh_max(double a, double b) { return (a > b || (a == b && std::signbit(b))) ? a : b; }
BVH_HD inline double bvh_half_area(const double *l, const double *h)
{
  const double dx = h[0] - l[0], dy = h[1] - l[1], dz = h[2] - l[2];
  return dx * dy + dy * dz + dz * dx;
}
/* box[0..2] = lo, box[3..5] = hi, cen[0..2] of the triangle g = (v0, e1, e2) */
BVH_HD inline void bvh_tri_box(const double *g, double *box, double *cen)
{
  for (int k = 0; k < 3; k++)
  {
    const double a = g[k], b = g[k] + g[3 + k], c = g[k] + g[6 + k];
    box[k] = bvh_min(a, bvh_min(b, c));
    box[3 + k] = bvh_max(a, bvh_max(b, c));
    cen[k] = (a + b + c) / 3.0;
  }
}
/* 64 bits that order as the finite doubles do, -0.0 and 0.0 alike */
BVH_HD inline uint64_t bvh_sort_key(double c)
{
  const double d = c + 0.0;
  uint64_t u;
  memcpy(&u, &d, sizeof u);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
BVH_HD inline double bvh_split_cost(double area_left, uint32_t i, double area_right, uint32_t m)
{
  return area_left * (double)i + area_right * (double)(m - i);
}

struct BvhSweep
{
  const double *tgeom = nullptr;   /* n_tri x 9: v0, e1, e2 */
  std::vector<uint32_t> order;     /* the final L0 */
  std::vector<double> nodes;       /* PT_BVH_SRC_DOUBLES per node, breadth-first */
  std::vector<double> box, cen;    /* per triangle: lo xyz hi xyz; centroid */
  std::vector<uint32_t> split_axis, split_left; /* per node: the winner (for the test that re-derives it) */
  int depth = 0, max_depth = 0;

  static double tree_cost_of(const std::vector<double> &nodes_in_order)
  {
    BvhBuild b;
    b.nodes = nodes_in_order;
    return b.tree_cost();
  }
  double tree_cost() const { return tree_cost_of(nodes); }

  void box_of(const std::vector<uint32_t> &list, uint32_t from, uint32_t to, double *out) const
  {
    for (int k = 0; k < 3; k++)
    {
      out[k] = HUGE_VAL;
      out[3 + k] = -HUGE_VAL;
    }
    for (uint32_t p = from; p < to; p++)
      for (int k = 0; k < 3; k++)
      {
        out[k] = bvh_min(out[k], box[6 * (size_t)list[p] + k]);
        out[3 + k] = bvh_max(out[3 + k], box[6 * (size_t)list[p] + 3 + k]);
      }
  }

  void build_root(uint32_t n)
  {
    max_depth = 0;
    while (((uint64_t)PT_BVH_LEAF << max_depth) < n)
      max_depth++;
    box.resize(6 * (size_t)n);
    cen.resize(3 * (size_t)n);
    for (uint32_t t = 0; t < n; t++)
      bvh_tri_box(tgeom + 9 * (size_t)t, &box[6 * (size_t)t], &cen[3 * (size_t)t]);
    std::vector<uint32_t> list[3];
    for (int a = 0; a < 3; a++)
    {
      list[a].resize(n);
      for (uint32_t t = 0; t < n; t++)
        list[a][t] = t;
      std::sort(list[a].begin(), list[a].end(), [&](uint32_t x, uint32_t y) {
        const uint64_t kx = bvh_sort_key(cen[3 * (size_t)x + a]), ky = bvh_sort_key(cen[3 * (size_t)y + a]);
        return kx != ky ? kx < ky : x < y;
      });
    }
    nodes.clear();
    split_axis.clear();
    split_left.clear();
    depth = 0;
    if (n <= PT_BVH_LEAF)
    { /* the root with the one leaf and an empty second one, as BvhBuild::build_tree makes it */
      nodes.assign(PT_BVH_SRC_DOUBLES, 0.0);
      box_of(list[0], 0, n, &nodes[0]);
      memcpy(&nodes[6], &nodes[0], 6 * sizeof(double));
      const uint32_t refs[2] = {PT_BVH_LEAF_FLAG | n, PT_BVH_LEAF_FLAG};
      memcpy(&nodes[12], refs, sizeof refs);
      depth = 1;
      order = list[0];
      return;
    }
    struct Range { uint32_t b, e; };
    std::vector<Range> level(1, Range{0, n}), next; /* the inner nodes of a level, left to right */
    std::vector<uint8_t> side(n, 0);
    std::vector<uint32_t> tmp(n);
    std::vector<double> area_l, area_r;
    uint32_t base = 0;
    for (int l = 0; !level.empty(); l++)
    {
      depth = l + 1;
      const uint64_t cap = (uint64_t)PT_BVH_LEAF << (max_depth - l - 1);
      const uint32_t next_base = base + (uint32_t)level.size();
      nodes.resize((size_t)next_base * PT_BVH_SRC_DOUBLES, 0.0);
      next.clear();
      for (size_t s = 0; s < level.size(); s++)
      {
        const uint32_t b = level[s].b, e = level[s].e, m = e - b;
        double best = HUGE_VAL;
        uint32_t best_axis = 0, best_i = m / 2;
        area_l.resize(m);
        area_r.resize(m);
        for (int a = 0; a < 3; a++)
        {
          double run[6] = {HUGE_VAL, HUGE_VAL, HUGE_VAL, -HUGE_VAL, -HUGE_VAL, -HUGE_VAL};
          for (uint32_t j = 0; j < m; j++) /* area_l[j]: the box of the first j + 1 */
          {
            const double *tb = &box[6 * (size_t)list[a][b + j]];
            for (int k = 0; k < 3; k++)
            {
              run[k] = bvh_min(run[k], tb[k]);
              run[3 + k] = bvh_max(run[3 + k], tb[3 + k]);
            }
            area_l[j] = bvh_half_area(run, run + 3);
          }
          for (int k = 0; k < 3; k++)
          {
            run[k] = HUGE_VAL;
            run[3 + k] = -HUGE_VAL;
          }
          for (uint32_t j = m; j-- > 0;) /* area_r[j]: the box of [j, m) */
          {
            const double *tb = &box[6 * (size_t)list[a][b + j]];
            for (int k = 0; k < 3; k++)
            {
              run[k] = bvh_min(run[k], tb[k]);
              run[3 + k] = bvh_max(run[3 + k], tb[3 + k]);
            }
            area_r[j] = bvh_half_area(run, run + 3);
          }
          for (uint32_t i = 1; i < m; i++)
          {
            if (i > cap || m - i > cap)
              continue;
            const double cost = bvh_split_cost(area_l[i - 1], i, area_r[i], m);
            if (cost < best)
            {
              best = cost;
              best_axis = (uint32_t)a;
              best_i = i;
            }
          }
        }
        split_axis.push_back(best_axis);
        split_left.push_back(best_i);
        for (uint32_t p = b; p < e; p++)
          side[list[best_axis][p]] = p >= b + best_i;
        for (int a = 0; a < 3; a++)
        {
          uint32_t zl = b, zr = b + best_i;
          for (uint32_t p = b; p < e; p++)
            tmp[side[list[a][p]] ? zr++ : zl++] = list[a][p];
          std::copy(tmp.begin() + b, tmp.begin() + e, list[a].begin() + b);
        }
        double *nd = &nodes[(size_t)(base + s) * PT_BVH_SRC_DOUBLES];
        uint32_t refs[2];
        const Range child[2] = {Range{b, b + best_i}, Range{b + best_i, e}};
        for (int c = 0; c < 2; c++)
        {
          box_of(list[0], child[c].b, child[c].e, nd + 6 * c);
          const uint32_t cm = child[c].e - child[c].b;
          if (cm <= PT_BVH_LEAF)
            refs[c] = PT_BVH_LEAF_FLAG | (child[c].b << PT_BVH_COUNT_BITS) | cm;
          else
          {
            refs[c] = next_base + (uint32_t)next.size();
            next.push_back(child[c]);
          }
        }
        memcpy(nd + 12, refs, sizeof refs);
      }
      base = next_base;
      level.swap(next);
    }
    order = list[0];
  }
};

/* ---- refitting a tree to moved triangles: same topology, same leaf order, new boxes ----
 * The contract of scene_update.hip's refit (rt_hip_scene_update_vertices), stated in sequential C++ and tested against the
 * device byte for byte (tests/bvh_refit_harness.cpp, tests/test_gpu_scene_update.py).  Input: a tree as rt_hip_scene_bvh_read
 * returns it, from either builder, and the new tgeom (n x 9: v0, e1, e2).  Only the box doubles of `nodes` are rewritten; the
 * refs, the padding and `order` stay.
 *   child = a leaf [b, b + count)   the join of bvh_tri_box(order[b + j]) over the leaf, started from (+inf, -inf)
 *   child = an inner node           the join of that node's two child boxes
 *   child = the empty leaf          (count 0: the second child of a one-leaf mesh's root) its six doubles stay as they are
 * The join uses bvh_min / bvh_max (-0.0 below 0.0), which are associative and commutative: a box does not depend on the order
 * its members were joined in, so any schedule -- this loop, the device's level sweep -- gives the same bytes.
 * Both builders number a child above its parent (BvhBuild: preorder; BvhSweep and the device: breadth-first), so one pass from
 * the last node to the first meets every node after its children; refit() asserts it, levels() reports a tree that breaks it. */
struct BvhRefit
{
  BVH_HD static uint32_t child_ref(const double *nodes, uint32_t node, int child)
  {
    uint32_t refs[2];
    memcpy(refs, nodes + (size_t)node * PT_BVH_SRC_DOUBLES + 12, sizeof refs);
    return refs[child];
  }
  BVH_HD static bool is_leaf(uint32_t ref) { return (ref & PT_BVH_LEAF_FLAG) != 0; }
  BVH_HD static uint32_t leaf_count(uint32_t ref) { return ref & ((1u << PT_BVH_COUNT_BITS) - 1u); }
  BVH_HD static uint32_t leaf_first(uint32_t ref) { return (ref & ~PT_BVH_LEAF_FLAG) >> PT_BVH_COUNT_BITS; }

  BVH_HD static void join(double *box, const double *other)
  {
    for (int k = 0; k < 3; k++)
    {
      box[k] = bvh_min(box[k], other[k]);
      box[3 + k] = bvh_max(box[3 + k], other[3 + k]);
    }
  }
  BVH_HD static void empty(double *box)
  {
    for (int k = 0; k < 3; k++)
    {
      box[k] = HUGE_VAL;
      box[3 + k] = -HUGE_VAL;
    }
  }
  /* the box of the leaf `ref` (count > 0) over the triangles order[first .. first + count) of tgeom */
  BVH_HD static void leaf_box(const double *tgeom, const uint32_t *order, uint32_t ref, double *box)
  {
    const uint32_t first = leaf_first(ref), count = leaf_count(ref);
    empty(box);
    for (uint32_t j = 0; j < count; j++)
    {
      double tb[6], cen[3];
      bvh_tri_box(tgeom + 9 * (size_t)order[first + j], tb, cen);
      join(box, tb);
    }
  }
  /* the box of the inner node `ref`, whose own child boxes are final */
  BVH_HD static void inner_box(const double *nodes, uint32_t ref, double *box)
  {
    const double *nd = nodes + (size_t)ref * PT_BVH_SRC_DOUBLES;
    empty(box);
    join(box, nd);
    join(box, nd + 6);
  }

  /* the restatement: nodes (n_nodes x PT_BVH_SRC_DOUBLES) refitted in place; false (and an assertion) where a child is not
   * numbered above its parent */
  static bool refit(double *nodes, size_t n_nodes, const uint32_t *order, const double *tgeom)
  {
    for (size_t i = n_nodes; i-- > 0;)
      for (int c = 0; c < 2; c++)
      {
        const uint32_t ref = child_ref(nodes, (uint32_t)i, c);
        double *box = nodes + i * PT_BVH_SRC_DOUBLES + 6 * c;
        if (is_leaf(ref))
        {
          if (leaf_count(ref) != 0)
            leaf_box(tgeom, order, ref, box);
          continue;
        }
        const bool child_above_parent = ref > i && ref < n_nodes;
        assert(child_above_parent);
        if (!child_above_parent)
          return false;
        inner_box(nodes, ref, box);
      }
    return true;
  }

  /* The topology's levels, which the device sweeps from the deepest to the root: by_level = the node numbers sorted by depth
   * (ascending within a level), level_begin[d] .. level_begin[d + 1] = the nodes of depth d.  Depends on the refs alone. */
  static bool levels(const double *nodes, size_t n_nodes, std::vector<uint32_t> &by_level, std::vector<uint32_t> &level_begin)
  {
    std::vector<uint32_t> depth(n_nodes, 0);
    uint32_t deepest = 0;
    for (size_t i = 0; i < n_nodes; i++)
      for (int c = 0; c < 2; c++)
      {
        const uint32_t ref = child_ref(nodes, (uint32_t)i, c);
        if (is_leaf(ref))
          continue;
        if (!(ref > i && ref < n_nodes))
          return false;
        depth[ref] = depth[i] + 1;
        deepest = std::max(deepest, depth[ref]);
      }
    level_begin.assign(n_nodes ? deepest + 2 : 1, 0);
    for (size_t i = 0; i < n_nodes; i++)
      level_begin[depth[i] + 1]++;
    for (size_t d = 1; d < level_begin.size(); d++)
      level_begin[d] += level_begin[d - 1];
    by_level.resize(n_nodes);
    std::vector<uint32_t> at(level_begin.begin(), level_begin.end());
    for (size_t i = 0; i < n_nodes; i++)
      by_level[at[depth[i]]++] = (uint32_t)i;
    return true;
  }
};

/* ---- the device builder (bvh_device.hip), as rt_hip_shim.hip calls it; HIP translation units only ---- */
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

/* A tree built on the current device.  `nodes` and `order` point into the build's one workspace allocation, which lives as
 * long as this object: the caller copies them to where the scene keeps them.  Not copyable. */
struct BvhDeviceTree
{
  void *workspace = nullptr;
  const double *nodes = nullptr;   /* n_nodes x PT_BVH_SRC_DOUBLES, breadth-first */
  const uint32_t *order = nullptr; /* n triangle indices: leaf order */
  uint32_t n_nodes = 0;
  int depth = 0, max_depth = 0;
  float build_ms = 0; /* device events around the build's kernels (the per-level read-back of a count included) */
  const char *failure = nullptr; /* set where bvh_device_build fails a consistency check of its own rather than a HIP call */
  BvhDeviceTree() = default;
  BvhDeviceTree(const BvhDeviceTree &) = delete;
  BvhDeviceTree &operator=(const BvhDeviceTree &) = delete;
  ~BvhDeviceTree()
  {
    if (workspace)
      (void)hipFree(workspace);
  }
};

/* Builds the tree over tri_geom (device memory, n x 9 doubles: v0, e1, e2; 0 < n < 2^(31 - PT_BVH_COUNT_BITS)) on the null
 * stream of the current device and waits for it.  hipErrorOutOfMemory when the workspace cannot be had. */
hipError_t bvh_device_build(const double *tri_geom, uint32_t n, BvhDeviceTree *out);

/* tri_geom_leaf[k] = tri_geom[order[k]] (9 doubles each), on the null stream; all three in device memory */
hipError_t bvh_device_gather_leaf(const double *tri_geom, const uint32_t *order, uint32_t n, double *tri_geom_leaf);
#endif /* __HIPCC__ */

/* ---- a scene's triangles moved in place (scene_update.hip, rt_hip_scene_update_vertices) ----
 * What a triangle's records are made of, in one text for the host (scene_create_impl, rt_hip_shim.hip) and the device
 * (k_update_triangles), and -- for HIP translation units only -- the interface of scene_update.hip.  Compiled with
 * -ffp-contract=off on both sides: the records of an updated scene equal a freshly created scene's bit for bit. */

/* One triangle (p0, p1, p2: xyz each): its tri_geom record g[9] = (v0, e1, e2) and its entry_src record b[PT_ENTRY_SRC_STRIDE],
 * the phase-1 bound: a sphere around the centroid through the farthest vertex, slightly enlarged; feeds the conservative filter
 * only, never a result. */
BVH_HD inline void scene_triangle_entry(const double *p0, const double *p1, const double *p2, double *g, double *b)
{
  for (int k = 0; k < 3; k++)
  {
    g[k] = p0[k];
    g[3 + k] = p1[k] - p0[k]; /* raytracer.c:132-133 */
    g[6 + k] = p2[k] - p0[k];
  }
  const double cen[3] = {(p0[0] + p1[0] + p2[0]) / 3.0, (p0[1] + p1[1] + p2[1]) / 3.0, (p0[2] + p1[2] + p2[2]) / 3.0};
  const double *vs[3] = {p0, p1, p2};
  double rb2 = 0;
  for (int j = 0; j < 3; j++)
  {
    const double dx = vs[j][0] - cen[0], dy = vs[j][1] - cen[1], dz = vs[j][2] - cen[2];
    rb2 = std::fmax(rb2, dx * dx + dy * dy + dz * dz);
  }
  const double rb = std::sqrt(rb2) * (1.0 + 1e-9) + 1e-300;
  b[0] = cen[0];
  b[1] = cen[1];
  b[2] = cen[2];
  b[3] = rb * rb;
  b[4] = std::sqrt(cen[0] * cen[0] + cen[1] * cen[1] + cen[2] * cen[2]) * (1.0 + 1e-12);
  b[5] = rb;
}

/* its tri_normal record: calculate_surface_normal :42-45, normalize(cross(v2 - v0, v1 - v0)); NaN for a degenerate triangle */
BVH_HD inline void scene_triangle_normal(const double *g, double *n)
{
  const double *e1 = g + 3, *e2 = g + 6;
  const double cx = e2[1] * e1[2] - e2[2] * e1[1], cy = e2[2] * e1[0] - e2[0] * e1[2], cz = e2[0] * e1[1] - e2[1] * e1[0];
  const double s = 1.0 / std::sqrt(cx * cx + cy * cy + cz * cz);
  n[0] = cx * s;
  n[1] = cy * s;
  n[2] = cz * s;
}

/* corner k (0, 1, 2) of the triangle as the kernels see it: v0, v0 + e1, v0 + e2 */
BVH_HD inline void scene_triangle_corner(const double *g, int k, double *p)
{
  for (int a = 0; a < 3; a++)
    p[a] = k == 0 ? g[a] : g[a] + g[3 * k + a];
}

/* What a scene derives from the bounds of its triangles' corners, in one text for rt_hip_scene_create and
 * rt_hip_scene_update_vertices (host code on both sides; tests/mesh_bounds_harness.cpp is its CPU test).  The two reductions --
 * lo, hi over the corners, then r2 = the largest squared distance of a corner from scene_mesh_centre(lo, hi) -- are the
 * caller's: a host loop at creation, scene_update_check and scene_update_triangles on the device. */
struct SceneMeshBounds
{
  double c[3] = {0, 0, 0}; /* bounding sphere of every triangle (bvh_probe): the middle of the corners' bounds */
  double R = -1;           /* its radius; < 0: no triangles */
  double c_norm = 0;       /* |c|, rounded up */
  bool round = false;      /* the sphere's silhouette is no larger than the mean silhouette of the triangles' box */
  double tau = -1;         /* the margin of pt_build_hull_flags; < 0: no hull flags */
};

inline void scene_mesh_centre(const double lo[3], const double hi[3], double c[3])
{
  for (int a = 0; a < 3; a++)
    c[a] = 0.5 * lo[a] + 0.5 * hi[a];
}

/* The radius is the farthest corner's distance with slack for the roundings of e1, e2 and of the exact test's own barycentric
 * limits; non-finite input gives a bound that keeps every ray (and `round` is whatever the comparison says: false for NaN).
 * tau = 2^-43 x the triangles' extent -- 64 u sigma_max extent with u = 2^-53 and the shape limit sigma_max = 16, well above the
 * residual of a facet's own corners and of coplanar neighbours (~u sigma extent) -- unless the extent is too large for it. */
inline void scene_mesh_bounds(const double lo[3], const double hi[3], double r2, SceneMeshBounds *b)
{
  scene_mesh_centre(lo, hi, b->c);
  b->R = std::sqrt(r2) * (1.0 + 1e-9) + 1e-300;
  if (!(b->R < HUGE_VAL))
    b->R = HUGE_VAL;
  b->c_norm = std::sqrt(b->c[0] * b->c[0] + b->c[1] * b->c[1] + b->c[2] * b->c[2]) * (1.0 + 1e-12);
  const double ea = hi[0] - lo[0], eb = hi[1] - lo[1], ec = hi[2] - lo[2], extent = b->c_norm + b->R;
  b->round = 3.14159265358979 * b->R * b->R <= 0.5 * (ea * eb + eb * ec + ec * ea);
  b->tau = b->R < 1e150 ? 1.1368683772161603e-13 * extent : -1.0;
}

/* ---- a scene's spheres moved in place (scene_update.hip, rt_hip_scene_update_spheres) ----
 * What a scene derives from its spheres, in one text for the host (scene_create_impl, rt_hip_shim.hip), the device
 * (k_update_spheres, scene_update.hip) and the CPU test of both (tests/sphere_update_harness.cpp, through scene_spheres.h).  Input
 * everywhere: 4 doubles a sphere, cx cy cz radius, in object order (the layout of rt_hip_scene_update_spheres and of
 * rt_hip_selftest_intersect kind 0).  Compiled with -ffp-contract=off on every side: the records and scalars of an updated scene
 * equal a freshly created scene's bit for bit.  Every scalar is a maximum (or an OR, the maximum of 0 and 1) over the spheres, or a
 * function of the leading eight records alone, so the device's reduction does not depend on the order its waves arrive in. */
#define SCENE_SPHERE_IN 4   /* doubles a sphere of the input: cx cy cz radius */
#define SCENE_SPHERE_WALLS 8 /* leading wall-sized spheres looked at: 2 PT_BIG_PAIRS */

/* One sphere's record of entry_src (pt_device.h): cx cy cz, r*r, |c| rounded up, 0 -- and, where asked for, its geom4 copy (the
 * first PT_GEOM_STRIDE doubles: what the exact test and the normal read). */
BVH_HD inline void scene_sphere_entry(const double *center, double radius, double *g, double *g4)
{
  g[0] = center[0];
  g[1] = center[1];
  g[2] = center[2];
  g[3] = radius * radius; /* raytracer.c:87 */
  /* |c|, rounded up: feeds the conservative phase-1 thresholds only, never a result */
  g[4] = std::sqrt(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]) * (1.0 + 1e-12);
  g[5] = 0.0; /* a sphere is rejected when its centre is behind the origin at all (raytracer.c:84) */
  if (g4)
    for (int k = 0; k < PT_GEOM_STRIDE; k++)
      g4[k] = g[k];
}

/* rt_hip_scene_create's rule for a radius (RT_HIP_ELIMIT otherwise); false for NaN */
BVH_HD inline bool scene_sphere_radius_ok(double radius) { return std::fabs(radius) >= 1e-100 && std::fabs(radius) <= 1e100; }

/* The sphere's part of each scalar; the scene's value is the maximum over the spheres, from 0.
 * reach_spheres: |c| + |r| of a sphere of ordinary size (wall-sized spheres would only loosen the filter).  fmax(0, x) is x for
 * every x a sphere can give (x >= 0, or +inf) and drops a NaN, as the host's running fmax(reach, x) does. */
BVH_HD inline double scene_sphere_reach_part(const double *g, double radius)
{
  return std::fabs(radius) < 1000.0 ? std::fmax(0.0, g[4] + std::fabs(radius)) : 0.0;
}
BVH_HD inline double scene_sphere_center_part(const double *g) { return std::fmax(0.0, g[4]); }
/* a centre or radius beyond 1e17 (or not a number): the scene takes the scalar-table _big kernels */
BVH_HD inline uint32_t scene_sphere_wide_part(const double *g, double radius)
{
  return (!(g[4] <= 1e17) || !(std::fabs(radius) <= 1e17)) ? 1u : 0u;
}
/* a wall-sized sphere that BigPrune (pt_filter.h) may use */
BVH_HD inline bool scene_sphere_is_wall(double radius) { return std::fabs(radius) >= 1000.0 && std::fabs(radius) <= 1e17; }

struct SceneSphereBounds
{
  double reach_spheres = 0; /* the spheres' part of the scene's reach */
  double max_center = 0;    /* max |centre| (rounded up) */
  uint32_t wide_range = 0;
  /* the LEADING wall-sized spheres, whole pairs of them, at most SCENE_SPHERE_WALLS: radius and |centre|; 0 from n_big on */
  uint32_t n_big = 0;
  double big_r[SCENE_SPHERE_WALLS] = {0}, big_c[SCENE_SPHERE_WALLS] = {0};
};

/* n_big, big_r, big_c from the leading records (spheres: 4 doubles each, n of them; only the first SCENE_SPHERE_WALLS are read) */
inline void scene_sphere_leading_walls(const double *spheres, size_t n, SceneSphereBounds *b)
{
  uint32_t nb = 0;
  double r[SCENE_SPHERE_WALLS], c[SCENE_SPHERE_WALLS];
  while (nb < SCENE_SPHERE_WALLS && (size_t)nb < n && scene_sphere_is_wall(spheres[SCENE_SPHERE_IN * (size_t)nb + 3]))
  {
    double g[PT_ENTRY_SRC_STRIDE];
    scene_sphere_entry(spheres + SCENE_SPHERE_IN * (size_t)nb, spheres[SCENE_SPHERE_IN * (size_t)nb + 3], g, nullptr);
    r[nb] = std::fabs(spheres[SCENE_SPHERE_IN * (size_t)nb + 3]);
    c[nb] = g[4];
    nb++;
  }
  b->n_big = nb & ~1u; /* whole pairs */
  for (uint32_t k = 0; k < SCENE_SPHERE_WALLS; k++)
  {
    b->big_r[k] = k < b->n_big ? r[k] : 0.0;
    b->big_c[k] = k < b->n_big ? c[k] : 0.0;
  }
}

/* The sequential statement of everything above: the records (entry: PT_ENTRY_SRC_STRIDE n doubles, geom4: PT_GEOM_STRIDE n; either
 * may be null) and the scalars of n spheres.  What scene_create_impl calls, and what the device's update is tested against. */
inline void scene_sphere_bounds(const double *spheres, size_t n, double *entry, double *geom4, SceneSphereBounds *b)
{
  *b = SceneSphereBounds();
  for (size_t i = 0; i < n; i++)
  {
    const double *s = spheres + SCENE_SPHERE_IN * i;
    double g[PT_ENTRY_SRC_STRIDE];
    scene_sphere_entry(s, s[3], g, geom4 ? geom4 + PT_GEOM_STRIDE * i : nullptr);
    if (entry)
      for (int k = 0; k < PT_ENTRY_SRC_STRIDE; k++)
        entry[PT_ENTRY_SRC_STRIDE * i + k] = g[k];
    b->reach_spheres = std::fmax(b->reach_spheres, scene_sphere_reach_part(g, s[3]));
    b->max_center = std::fmax(b->max_center, scene_sphere_center_part(g));
    b->wide_range |= scene_sphere_wide_part(g, s[3]);
  }
  scene_sphere_leading_walls(spheres, n, b);
}

/* ---- a scene's materials changed in place (scene_update.hip, rt_hip_scene_update_materials) ----
 * What a scene derives from its materials, in one text for the host (scene_create_impl, rt_hip_shim.hip), the device
 * (k_update_materials, scene_update.hip) and the CPU test of both (tests/material_harness.cpp, through scene_materials.h): the
 * `material` record of PT_MAT_STRIDE doubles an object, its `color_raw` triple, and the object's part of four scalars --
 * max_emission (a maximum) and the three flag classes any_refract, any_checker, any_mirror_glass (ORs).  Input everywhere: 6
 * doubles an object, colour then emission, and the object's flags; objects in rt_hip_scene_create's numbering, spheres first,
 * mesh m at n_spheres + m.  Compiled with -ffp-contract=off on every side: records and scalars of an updated scene equal a
 * freshly created scene's bit for bit -- with ONE exception that no kernel can see: a black colour gives prob = 0, inv = +inf and
 * 0 * inf = NaN in doubles 1..3, and the sign bit of that default NaN is the machine's (host and device may differ).  The
 * reference never reads the three (`random_double() < 0` is false, raytracer.c:497-500), so a comparison of records takes a NaN
 * as equal to a NaN and every other word by its bits. */
#define SCENE_MATERIAL_IN 6 /* doubles an object of the input: colour rgb, emission rgb */

/* rt_hip_scene_create's rule (RT_HIP_EINVAL otherwise): the pooled kernels' fixed-point sums rest on throughput <= 1, i.e. on
 * albedo / MAX(albedo) in [0, 1] -- colours finite and non-negative (-0.0 is), at most 1e100; |emission| at most 1e100.  False
 * for a NaN anywhere. */
BVH_HD inline bool scene_material_ok(const double *color, const double *emission)
{
  for (int k = 0; k < 3; k++)
    if (!(color[k] >= 0.0) || !(color[k] <= 1e100) || !(std::fabs(emission[k]) <= 1e100))
      return false;
  return true;
}

/* One object's record (pt_device.h): prob, albedo / prob, emission, the flags as the uint64 bit pattern of double 7 */
BVH_HD inline void scene_material_record(uint32_t flags, const double *color, const double *emission, double *m)
{
  /* raytracer.c:497: prob = MAX(albedo.x, MAX(albedo.y, albedo.z)) */
  const double yz = color[1] > color[2] ? color[1] : color[2];
  const double prob = color[0] > yz ? color[0] : yz;
  const double inv = 1 / prob; /* :500 vec3_scalar_mult(albedo, 1 / prob) */
  m[0] = prob;
  m[1] = color[0] * inv;
  m[2] = color[1] * inv;
  m[3] = color[2] * inv;
  m[4] = emission[0];
  m[5] = emission[1];
  m[6] = emission[2];
  const uint64_t bits = flags;
  memcpy(&m[7], &bits, sizeof bits);
}
/* the flags a record holds (an update without flags keeps them) */
BVH_HD inline uint32_t scene_material_flags(const double *m)
{
  uint64_t bits;
  memcpy(&bits, &m[7], sizeof bits);
  return (uint32_t)bits;
}

/* The object's part of each scalar.  max_emission: the scene's value is the maximum over the objects, from 0 (material_ok has
 * ruled out a NaN). */
BVH_HD inline double scene_material_emission_part(const double *emission)
{
  return std::fmax(std::fabs(emission[0]), std::fmax(std::fabs(emission[1]), std::fabs(emission[2])));
}
/* the flag classes, one bit each; the scene's value is the OR over the objects */
#define SCENE_MATERIAL_REFRACT 1u      /* view.any_refract: an M_REFRACTION material */
#define SCENE_MATERIAL_CHECKER 2u      /* view.any_checker: an M_CHECKERED material */
#define SCENE_MATERIAL_MIRROR_GLASS 4u /* any_mirror_glass: M_REFLECTION and M_REFRACTION on one object */
BVH_HD inline uint32_t scene_material_class_part(uint32_t flags)
{
  const uint32_t both = PT_FLAG_MIRROR | PT_FLAG_REFRACT;
  return ((flags & PT_FLAG_REFRACT) ? SCENE_MATERIAL_REFRACT : 0u) | ((flags & PT_FLAG_CHECKER) ? SCENE_MATERIAL_CHECKER : 0u) |
         ((flags & both) == both ? SCENE_MATERIAL_MIRROR_GLASS : 0u);
}

struct SceneMaterialBounds
{
  double max_emission = 0; /* max |emission component| over the objects */
  uint32_t classes = 0;    /* SCENE_MATERIAL_* of any object */
};

/* The sequential statement of everything above for n objects that material_ok accepts: the records (material: PT_MAT_STRIDE n
 * doubles), the colours as given (color_raw: 3 n; either may be null) and the scalars.  in: SCENE_MATERIAL_IN doubles an object.
 * What scene_create_impl calls, and what the device's update is tested against. */
inline void scene_material_bounds(const double *in, const uint32_t *flags, size_t n, double *material, double *color_raw, SceneMaterialBounds *b)
{
  *b = SceneMaterialBounds();
  for (size_t i = 0; i < n; i++)
  {
    const double *c = in + SCENE_MATERIAL_IN * i, *e = c + 3;
    if (material)
      scene_material_record(flags[i], c, e, material + PT_MAT_STRIDE * i);
    if (color_raw)
      for (int k = 0; k < 3; k++)
        color_raw[3 * i + k] = c[k];
    b->max_emission = std::fmax(b->max_emission, scene_material_emission_part(e));
    b->classes |= scene_material_class_part(flags[i]);
  }
}

/* ---- a tree priced on the device (scene_update.hip: k_tree_cost; rt_hip_scene_bvh_cost, rt_hip.h states the contract) ----
 * BvhBuild::tree_cost()'s formula, term by term, in one text for the kernel and for whoever restates it on the host: the terms
 * are the same doubles; only the order of the additions differs (a fixed tree here, node order there).  fp64, unfused
 * (-ffp-contract=off), in the order written. */
#define BVH_COST_BLOCK 256 /* terms a block of the reduction tree takes */
/* the half area of the root's box, from node 0: NaN components of one child's box give way to the other's (fmin / fmax) */
BVH_HD inline double bvh_cost_root_area(const double *n0)
{
  double lo[3], hi[3];
  for (int k = 0; k < 3; k++)
  {
    lo[k] = std::fmin(n0[k], n0[6 + k]);
    hi[k] = std::fmax(n0[3 + k], n0[9 + k]);
  }
  return bvh_half_area(lo, hi);
}
BVH_HD inline bool bvh_cost_root_ok(double a_root) { return a_root > 0 && a_root < 1e300; }
/* node n's term (c0 + c1): an empty leaf child is +0.0, another child (half_area / a_root) * (leaf ? 45 count : 60) */
BVH_HD inline double bvh_cost_term(const double *n, double a_root)
{
  uint32_t refs[2];
  memcpy(refs, n + 12, sizeof refs);
  double c[2];
  for (int k = 0; k < 2; k++)
  {
    const bool leaf = (refs[k] & PT_BVH_LEAF_FLAG) != 0;
    const uint32_t count = refs[k] & ((1u << PT_BVH_COUNT_BITS) - 1u);
    c[k] = (leaf && count == 0) ? 0.0 : (bvh_half_area(n + 6 * k, n + 6 * k + 3) / a_root) * (leaf ? 45.0 * (double)count : 60.0);
  }
  return c[0] + c[1];
}

#if defined(__HIPCC__)

/* the arrays of a scene that an update rewrites (device memory) */
struct SceneUpdateArrays
{
  uint32_t n_tri = 0, n_nodes = 0;
  double *tri_geom = nullptr, *tri_normal = nullptr; /* 9 n, 3 n */
  double *entry_tri = nullptr;                       /* the triangles' part of entry_src: PT_ENTRY_SRC_STRIDE n */
  uint32_t *tri_object = nullptr;                    /* n: the hull bits are cleared */
  double *bvh_src = nullptr;                         /* n_nodes x PT_BVH_SRC_DOUBLES: the boxes are rewritten */
  const uint32_t *bvh_tri = nullptr;                 /* n: the leaf order */
  double *tri_geom_leaf = nullptr;                   /* 9 n */
};

/* what k_check_positions reduces, as the host reads it back */
struct SceneUpdateCheck
{
  double max_len;      /* max |vertex| over the 3 n positions; +infinity where one is not <= 1e300 (NaN included) */
  double lo[3], hi[3]; /* bounds of the corners as the kernels see them, joined by bvh_min / bvh_max */
};
#define SCENE_UPDATE_WORDS 8 /* 64-bit words of device workspace the reductions need: 7 of the check, 1 of r^2 */

/* All on the null stream of the current device; positions = 9 doubles a triangle (v0, v1, v2) in device memory.
 * scene_update_check reads the positions alone, writes `words` alone and waits for the result. */
hipError_t scene_update_check(const double *positions, uint32_t n_tri, unsigned long long *words, SceneUpdateCheck *out);
/* tri_geom, tri_normal, the entry records, tri_object's hull bits; *r2 = the largest squared distance of a corner from mesh_c
 * (waits for it) */
hipError_t scene_update_triangles(const SceneUpdateArrays &s, const double *positions, const double mesh_c[3],
                                  unsigned long long *words, double *r2);
/* BvhRefit on the device: the leaf children, then the inner ones level by level from the deepest (by_level in device memory,
 * level_begin on the host: BvhRefit::levels), and tri_geom_leaf.  Enqueues only. */
hipError_t scene_update_refit(const SceneUpdateArrays &s, const uint32_t *by_level, const uint32_t *level_begin, size_t n_levels);

/* doubles of device workspace the cost of n_nodes nodes needs: a sum per block of nodes, and a sum per block of those */
inline size_t scene_tree_cost_ws_doubles(uint32_t n_nodes)
{
  const size_t b1 = ((size_t)n_nodes + BVH_COST_BLOCK - 1) / BVH_COST_BLOCK;
  return b1 + (b1 + BVH_COST_BLOCK - 1) / BVH_COST_BLOCK;
}
/* The cost of a tree by the contract above (k_tree_cost, scene_update.hip): nodes = n_nodes x PT_BVH_SRC_DOUBLES in device memory
 * of the current device.  Null stream; ws = scene_tree_cost_ws_doubles(n_nodes) doubles of device memory the caller keeps (a
 * scene keeps one: no allocation in a per-frame question), or nullptr: the call allocates and frees them (hipErrorOutOfMemory
 * where they cannot be had).  Waits, and reads back the 8 bytes of the result.  n_nodes == 0: 0.0, nothing launched. */
hipError_t scene_tree_cost(const double *nodes, uint32_t n_nodes, double *ws, double *cost);

/* ---- the interface of scene_update.hip's sphere half (rt_hip_scene_update_spheres) ----
 * Both on the null stream of the current device; spheres = 4 doubles a sphere in device memory; words: SCENE_SPHERE_WORDS 64-bit
 * words of device workspace. */
#define SCENE_SPHERE_WORDS 4
/* reads the spheres alone, writes `words` alone and waits: the scalars that are maxima (n_big, big_r, big_c are not set) and
 * whether every radius is acceptable */
hipError_t scene_update_spheres_check(const double *spheres, uint32_t n, unsigned long long *words, SceneSphereBounds *out, bool *radii_ok);
/* writes the n records of entry (PT_ENTRY_SRC_STRIDE n) and geom4 (PT_GEOM_STRIDE n): the same kernel with its outputs given and
 * no words -- it reduces nothing.  Enqueues only. */
hipError_t scene_update_spheres_write(const double *spheres, uint32_t n, double *entry, double *geom4);

/* ---- the interface of scene_update.hip's material half (rt_hip_scene_update_materials) ----
 * Both on the null stream of the current device; in = SCENE_MATERIAL_IN doubles an object, flags = a word an object or nullptr
 * (every object keeps the flags of its record), both in device memory; words: SCENE_MATERIAL_WORDS 64-bit words of workspace. */
#define SCENE_MATERIAL_WORDS 5
/* reads the input and, without flags, double 7 of the n records at `present`; writes `words` alone and waits: the scalars, and
 * whether scene_material_ok accepts every object (max_emission then leaves the refused ones out) */
hipError_t scene_update_materials_check(const double *in, const uint32_t *flags, uint32_t n, const double *present,
                                        unsigned long long *words, SceneMaterialBounds *out, bool *materials_ok);
/* writes the n records of material (PT_MAT_STRIDE n; without flags each keeps its own) and color_raw (3 n): the same kernel with
 * its outputs given and no words -- it reduces nothing.  Enqueues only. */
hipError_t scene_update_materials_write(const double *in, const uint32_t *flags, uint32_t n, double *material, double *color_raw);
#endif /* __HIPCC__ */

#endif /* BVH_BUILD_H */

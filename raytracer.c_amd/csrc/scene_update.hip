/* scene_update.hip -- a scene's triangles moved in place (rt_hip_scene_update_vertices): every per-triangle record the kernels
 * read is recomputed on the device from new positions, and the existing hierarchy is refitted -- same topology, same leaf order,
 * new boxes.  The contracts are bvh_build.h's scene_triangle_* inlines (the records: one text with scene_create_impl) and BvhRefit
 * (bvh_build.h: the boxes); both are met bit for bit, which rests on -ffp-contract=off and on reductions that are maxima and
 * minima only -- no result depends on the order threads arrive in.
 *   k_check_positions    max |vertex| and the bounds of the corners: reads the positions, writes seven words, nothing of the scene
 *   k_update_triangles   tri_geom, tri_normal, the entry_src records, tri_object's hull bits cleared; max r^2 about the new centre
 *   k_refit_leaves       one thread a child slot: the box of a leaf child from tri_geom through bvh_tri
 *   k_refit_level        one thread a child slot of one level's nodes: the box of an inner child from that node's two boxes;
 *                        launched level by level from the deepest, so every launch reads boxes an earlier one finished
 *   tri_geom_leaf        bvh_device_gather_leaf
 * and a scene's spheres moved in place (rt_hip_scene_update_spheres; the contract is scene_spheres.h's scene_sphere_bounds):
 *   k_update_spheres     one thread a sphere: the entry_src record and its geom4 copy (where an output is given), and the maxima
 *                        the scene keeps of its spheres -- reach, max |centre|, wide range -- with "a radius is out of range"
 * and a scene's materials changed in place (rt_hip_scene_update_materials; the contract is scene_materials.h's scene_material_bounds):
 *   k_update_materials   one thread an object: the `material` record and the color_raw triple (where an output is given), and what
 *                        the scene keeps of its materials -- max |emission|, the three flag classes -- with "a material is not
 *                        acceptable"
 * and a tree priced where it lies (rt_hip_scene_bvh_cost; the contract is bvh_build.h's bvh_cost_* and rt_hip.h):
 *   k_tree_cost          one level of a fixed reduction tree over the nodes' cost terms, launched level by level from the host
 * 256 threads a workgroup, no scratch, no LDS (k_tree_cost: 2 KB, for its two widest halvings); no kernel waits for another
 * workgroup: a wave reduces by lane shuffles and hands its result to one atomic max / min on a 64-bit key (k_tree_cost: to its
 * block's own slot -- a sum has no atomics here). */
#include <hip/hip_runtime.h>

#include <cstring>

#include "bvh_build.h"
#include "scene_materials.h"
#include "scene_spheres.h"

namespace
{

constexpr int UPD_BLOCK = 256;
constexpr uint32_t UPD_CHECK_BLOCKS = 1024; /* k_check_positions strides over the triangles: at most 4096 waves meet the atomics */

/* 64 bits that order as the doubles do, -0.0 below 0.0 (the order of bvh_min / bvh_max) */
__host__ __device__ inline unsigned long long key_of(double d)
{
  unsigned long long u;
  memcpy(&u, &d, sizeof u);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__host__ __device__ inline double double_of(unsigned long long k)
{
  const unsigned long long u = (k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k;
  double d;
  memcpy(&d, &u, sizeof d);
  return d;
}

__device__ inline unsigned long long wave_max(unsigned long long k)
{
  for (int d = 32; d >= 1; d >>= 1)
  {
    const unsigned long long o = __shfl_xor(k, d);
    k = o > k ? o : k;
  }
  return k;
}
__device__ inline unsigned long long wave_min(unsigned long long k)
{
  for (int d = 32; d >= 1; d >>= 1)
  {
    const unsigned long long o = __shfl_xor(k, d);
    k = o < k ? o : k;
  }
  return k;
}

/* words[0] = key of max |vertex|, words[1..3] = keys of lo, words[4..6] = keys of hi */
__global__ void __launch_bounds__(UPD_BLOCK) k_check_positions(const double *__restrict__ positions, uint32_t n,
                                                              unsigned long long *__restrict__ words)
{
  double len = 0.0, lo[3] = {HUGE_VAL, HUGE_VAL, HUGE_VAL}, hi[3] = {-HUGE_VAL, -HUGE_VAL, -HUGE_VAL};
  for (uint32_t t = blockIdx.x * UPD_BLOCK + threadIdx.x; t < n; t += gridDim.x * UPD_BLOCK)
  {
    double p[9], g[9], b[PT_ENTRY_SRC_STRIDE];
    for (int k = 0; k < 9; k++)
      p[k] = positions[9 * (size_t)t + k];
    for (int j = 0; j < 3; j++)
    {
      const double *q = p + 3 * j;
      const double l = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]);
      len = (l <= 1e300) ? std::fmax(len, l) : HUGE_VAL; /* NaN and what lies beyond the limit alike */
    }
    scene_triangle_entry(p, p + 3, p + 6, g, b);
    for (int j = 0; j < 3; j++)
    {
      double c[3];
      scene_triangle_corner(g, j, c);
      for (int a = 0; a < 3; a++)
      {
        lo[a] = bvh_min(lo[a], c[a]);
        hi[a] = bvh_max(hi[a], c[a]);
      }
    }
  }
  const unsigned long long kl = wave_max(key_of(len));
  unsigned long long klo[3], khi[3];
  for (int a = 0; a < 3; a++)
  {
    klo[a] = wave_min(key_of(lo[a]));
    khi[a] = wave_max(key_of(hi[a]));
  }
  if ((threadIdx.x & 63) == 0)
  {
    atomicMax(&words[0], kl);
    for (int a = 0; a < 3; a++)
    {
      atomicMin(&words[1 + a], klo[a]);
      atomicMax(&words[4 + a], khi[a]);
    }
  }
}

/* word[0] = key of the largest squared distance of a corner from (cx, cy, cz) */
__global__ void __launch_bounds__(UPD_BLOCK) k_update_triangles(SceneUpdateArrays s, const double *__restrict__ positions, double cx,
                                                               double cy, double cz, unsigned long long *__restrict__ word)
{
  const uint32_t t = blockIdx.x * UPD_BLOCK + threadIdx.x;
  double r2 = 0.0;
  if (t < s.n_tri)
  {
    double p[9], g[9], b[PT_ENTRY_SRC_STRIDE], nrm[3];
    for (int k = 0; k < 9; k++)
      p[k] = positions[9 * (size_t)t + k];
    scene_triangle_entry(p, p + 3, p + 6, g, b);
    scene_triangle_normal(g, nrm);
    for (int k = 0; k < 9; k++)
      s.tri_geom[9 * (size_t)t + k] = g[k];
    for (int k = 0; k < 3; k++)
      s.tri_normal[3 * (size_t)t + k] = nrm[k];
    for (int k = 0; k < PT_ENTRY_SRC_STRIDE; k++)
      s.entry_tri[PT_ENTRY_SRC_STRIDE * (size_t)t + k] = b[k];
    s.tri_object[t] &= ~(PT_HULL_PLUS | PT_HULL_MINUS);
    for (int j = 0; j < 3; j++)
    {
      double c[3];
      scene_triangle_corner(g, j, c);
      const double dx = c[0] - cx, dy = c[1] - cy, dz = c[2] - cz;
      r2 = std::fmax(r2, dx * dx + dy * dy + dz * dz);
    }
  }
  const unsigned long long k = wave_max(key_of(r2));
  if ((threadIdx.x & 63) == 0)
    atomicMax(word, k);
}

__device__ inline void store_box(double *to, const double *box)
{
  for (int k = 0; k < 6; k++)
    to[k] = box[k];
}

__global__ void __launch_bounds__(UPD_BLOCK) k_refit_leaves(SceneUpdateArrays s)
{
  const uint32_t slot = blockIdx.x * UPD_BLOCK + threadIdx.x;
  if (slot >= 2u * s.n_nodes)
    return;
  const uint32_t node = slot >> 1, c = slot & 1u;
  const uint32_t ref = BvhRefit::child_ref(s.bvh_src, node, (int)c);
  if (!BvhRefit::is_leaf(ref) || BvhRefit::leaf_count(ref) == 0)
    return;
  if (BvhRefit::leaf_first(ref) + BvhRefit::leaf_count(ref) > s.n_tri)
    return; /* (no tree of either builder has such a leaf: nothing is read past the order) */
  double box[6];
  BvhRefit::leaf_box(s.tri_geom, s.bvh_tri, ref, box);
  store_box(s.bvh_src + (size_t)node * PT_BVH_SRC_DOUBLES + 6 * c, box);
}

/* the nodes by_level[begin .. end): their inner children's boxes, from nodes one level down */
__global__ void __launch_bounds__(UPD_BLOCK) k_refit_level(SceneUpdateArrays s, const uint32_t *__restrict__ by_level, uint32_t begin,
                                                          uint32_t end)
{
  const uint32_t slot = blockIdx.x * UPD_BLOCK + threadIdx.x;
  if (slot >= 2u * (end - begin))
    return;
  const uint32_t node = by_level[begin + (slot >> 1)], c = slot & 1u;
  if (node >= s.n_nodes)
    return;
  const uint32_t ref = BvhRefit::child_ref(s.bvh_src, node, (int)c);
  if (BvhRefit::is_leaf(ref) || ref >= s.n_nodes)
    return;
  double box[6];
  BvhRefit::inner_box(s.bvh_src, ref, box);
  store_box(s.bvh_src + (size_t)node * PT_BVH_SRC_DOUBLES + 6 * c, box);
}

/* words[0] = key of reach_spheres, words[1] = key of max_center, words[2] = wide_range, words[3] = a radius is out of range.
 * entry == nullptr: nothing but the words is written (the check before anything of the scene changes); words == nullptr: nothing
 * is reduced (the write after it). */
__global__ void __launch_bounds__(UPD_BLOCK) k_update_spheres(const double *__restrict__ spheres, uint32_t n, double *__restrict__ entry,
                                                             double *__restrict__ geom4, unsigned long long *__restrict__ words)
{
  const uint32_t i = blockIdx.x * UPD_BLOCK + threadIdx.x;
  double reach = 0.0, center = 0.0;
  unsigned long long wide = 0, bad = 0;
  if (i < n)
  {
    double s[SCENE_SPHERE_IN], g[PT_ENTRY_SRC_STRIDE], g4[PT_GEOM_STRIDE];
    for (int k = 0; k < SCENE_SPHERE_IN; k++)
      s[k] = spheres[SCENE_SPHERE_IN * (size_t)i + k];
    scene_sphere_entry(s, s[3], g, g4);
    if (entry)
    {
      for (int k = 0; k < PT_ENTRY_SRC_STRIDE; k++)
        entry[PT_ENTRY_SRC_STRIDE * (size_t)i + k] = g[k];
      for (int k = 0; k < PT_GEOM_STRIDE; k++)
        geom4[PT_GEOM_STRIDE * (size_t)i + k] = g4[k];
    }
    reach = scene_sphere_reach_part(g, s[3]);
    center = scene_sphere_center_part(g);
    wide = scene_sphere_wide_part(g, s[3]);
    bad = scene_sphere_radius_ok(s[3]) ? 0u : 1u;
  }
  if (!words)
    return; /* the write run: the check run has reduced already (a kernel argument: the whole grid takes this way) */
  const unsigned long long kr = wave_max(key_of(reach)), kc = wave_max(key_of(center)), kw = wave_max(wide), kb = wave_max(bad);
  if ((threadIdx.x & 63) == 0)
  {
    atomicMax(&words[0], kr);
    atomicMax(&words[1], kc);
    atomicMax(&words[2], kw);
    atomicMax(&words[3], kb);
  }
}

/* words[0] = key of max_emission, words[1..3] = an object is of the class (M_REFRACTION; M_CHECKERED; M_REFLECTION and
 * M_REFRACTION), words[4] = a material is not acceptable.  in: SCENE_MATERIAL_IN doubles an object; flags: a word an object, or
 * nullptr: every object keeps the flags of its present record (double 7 of `present`, the scene's records).  material == nullptr:
 * nothing but the words is written (the check before anything of the scene changes); words == nullptr: nothing is reduced (the
 * write after it).  The write run's `material` is `present`: a thread reads its own record's flags before it stores the record. */
__global__ void __launch_bounds__(UPD_BLOCK) k_update_materials(const double *__restrict__ in, const uint32_t *__restrict__ flags, uint32_t n,
                                                               const double *present, double *material, double *__restrict__ color_raw,
                                                               unsigned long long *__restrict__ words)
{
  const uint32_t i = blockIdx.x * UPD_BLOCK + threadIdx.x;
  double emit = 0.0;
  unsigned long long refr = 0, chk = 0, glass2 = 0, bad = 0;
  if (i < n)
  {
    double c[SCENE_MATERIAL_IN], m[PT_MAT_STRIDE];
    for (int k = 0; k < SCENE_MATERIAL_IN; k++)
      c[k] = in[SCENE_MATERIAL_IN * (size_t)i + k];
    const uint32_t f = flags ? flags[i] : scene_material_flags(present + PT_MAT_STRIDE * (size_t)i);
    if (material)
    {
      scene_material_record(f, c, c + 3, m);
      for (int k = 0; k < PT_MAT_STRIDE; k++)
        material[PT_MAT_STRIDE * (size_t)i + k] = m[k];
      for (int k = 0; k < 3; k++)
        color_raw[3 * (size_t)i + k] = c[k];
    }
    bad = scene_material_ok(c, c + 3) ? 0u : 1u;
    emit = bad ? 0.0 : scene_material_emission_part(c + 3); /* (a refused update takes no scalar; a NaN has no key) */
    const uint32_t cls = scene_material_class_part(f);
    refr = (cls & SCENE_MATERIAL_REFRACT) ? 1u : 0u;
    chk = (cls & SCENE_MATERIAL_CHECKER) ? 1u : 0u;
    glass2 = (cls & SCENE_MATERIAL_MIRROR_GLASS) ? 1u : 0u;
  }
  if (!words)
    return; /* the write run: the check run has reduced already (a kernel argument: the whole grid takes this way) */
  const unsigned long long ke = wave_max(key_of(emit)), kr = wave_max(refr), kc = wave_max(chk), kg = wave_max(glass2), kb = wave_max(bad);
  if ((threadIdx.x & 63) == 0)
  {
    atomicMax(&words[0], ke);
    atomicMax(&words[1], kr);
    atomicMax(&words[2], kc);
    atomicMax(&words[3], kg);
    atomicMax(&words[4], kb);
  }
}

/* One level of the cost's reduction tree (bvh_build.h: bvh_cost_*; rt_hip.h states the contract).  in == nullptr: the first level,
 * term i is node i's, one node a thread, read once as two 64-byte halves; otherwise term i = in[i].  Terms from n on are +0.0.
 * out[block] = the block's sum by halving: v[i] = v[i] + v[i + m] for i < m, m = 128 and 64 through LDS, 32 .. 1 by lane shuffles
 * in the first wave.  The launch of one workgroup is the last level: it writes the cost, 60 + total, or 0.0 where the root's
 * area is not in (0, 1e300).  Every thread derives the root's area from node 0 (a uniform read); nothing depends on the order
 * workgroups or waves run in. */
typedef double cost_d2 __attribute__((ext_vector_type(2)));

__global__ void __launch_bounds__(BVH_COST_BLOCK) k_tree_cost(const double *__restrict__ nodes, uint32_t n_nodes,
                                                             const double *__restrict__ in, uint32_t n, double *__restrict__ out)
{
  static_assert(BVH_COST_BLOCK == 256 && PT_BVH_SRC_DOUBLES == 16, "four waves a block, 128 bytes a node");
  __shared__ double s_v[BVH_COST_BLOCK];
  const uint32_t t = threadIdx.x, i = blockIdx.x * BVH_COST_BLOCK + t;
  double n0[12];
  for (int k = 0; k < 12; k++)
    n0[k] = nodes[k];
  const double a_root = bvh_cost_root_area(n0);
  double v = 0.0;
  if (i < n)
  {
    if (in)
      v = in[i];
    else if (i < n_nodes)
    {
      const cost_d2 *p = reinterpret_cast<const cost_d2 *>(nodes + (size_t)i * PT_BVH_SRC_DOUBLES);
      double nd[PT_BVH_SRC_DOUBLES];
      for (int h = 0; h < 2; h++) /* the two halves */
        for (int k = 0; k < 4; k++)
        {
          const cost_d2 q = __builtin_nontemporal_load(p + 4 * h + k);
          nd[8 * h + 2 * k] = q.x;
          nd[8 * h + 2 * k + 1] = q.y;
        }
      v = bvh_cost_term(nd, a_root);
    }
  }
  s_v[t] = v;
  __syncthreads();
  if (t < 128)
    v = v + s_v[t + 128];
  if (t >= 64 && t < 128)
    s_v[t] = v; /* (no thread reads below 128 in the step above) */
  __syncthreads();
  if (t >= 64)
    return;
  v = v + s_v[t + 64];
  for (int m = 32; m >= 1; m >>= 1)
    v = v + __shfl_down(v, m); /* lane i < m is the tree's v[i]; the lanes from m on hold values nobody reads */
  if (t == 0)
    out[blockIdx.x] = gridDim.x != 1 ? v : bvh_cost_root_ok(a_root) ? 60.0 + v : 0.0;
}

#define UPD_TRY(expr)             \
  do                              \
  {                               \
    const hipError_t e_ = (expr); \
    if (e_ != hipSuccess)         \
      return e_;                  \
  } while (0)

} // namespace

hipError_t scene_update_check(const double *positions, uint32_t n_tri, unsigned long long *words, SceneUpdateCheck *out)
{
  if (!positions || !words || !out || n_tri == 0)
    return hipErrorInvalidValue;
  unsigned long long h[7];
  h[0] = key_of(0.0);
  for (int a = 0; a < 3; a++)
  {
    h[1 + a] = key_of(HUGE_VAL);
    h[4 + a] = key_of(-HUGE_VAL);
  }
  UPD_TRY(hipMemcpy(words, h, sizeof h, hipMemcpyHostToDevice));
  const uint32_t blocks = (n_tri + UPD_BLOCK - 1) / UPD_BLOCK;
  hipLaunchKernelGGL(k_check_positions, dim3(blocks < UPD_CHECK_BLOCKS ? blocks : UPD_CHECK_BLOCKS), dim3(UPD_BLOCK), 0, nullptr,
                     positions, n_tri, words);
  UPD_TRY(hipGetLastError());
  UPD_TRY(hipMemcpy(h, words, sizeof h, hipMemcpyDeviceToHost));
  out->max_len = double_of(h[0]);
  for (int a = 0; a < 3; a++)
  {
    out->lo[a] = double_of(h[1 + a]);
    out->hi[a] = double_of(h[4 + a]);
  }
  return hipSuccess;
}

hipError_t scene_update_triangles(const SceneUpdateArrays &s, const double *positions, const double mesh_c[3],
                                  unsigned long long *words, double *r2)
{
  if (!positions || !words || !r2 || s.n_tri == 0)
    return hipErrorInvalidValue;
  unsigned long long h = key_of(0.0);
  UPD_TRY(hipMemcpy(words + 7, &h, sizeof h, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_update_triangles, dim3((s.n_tri + UPD_BLOCK - 1) / UPD_BLOCK), dim3(UPD_BLOCK), 0, nullptr, s, positions,
                     mesh_c[0], mesh_c[1], mesh_c[2], words + 7);
  UPD_TRY(hipGetLastError());
  UPD_TRY(hipMemcpy(&h, words + 7, sizeof h, hipMemcpyDeviceToHost));
  *r2 = double_of(h);
  return hipSuccess;
}

hipError_t scene_update_refit(const SceneUpdateArrays &s, const uint32_t *by_level, const uint32_t *level_begin, size_t n_levels)
{
  if (s.n_tri == 0 || s.n_nodes == 0 || !by_level || !level_begin || n_levels == 0)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_refit_leaves, dim3((2u * s.n_nodes + UPD_BLOCK - 1) / UPD_BLOCK), dim3(UPD_BLOCK), 0, nullptr, s);
  for (size_t d = n_levels - 1; d-- > 0;) /* (the deepest level's children are leaves all) */
  {
    const uint32_t begin = level_begin[d], end = level_begin[d + 1];
    if (end <= begin || end > s.n_nodes)
      return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_refit_level, dim3((2u * (end - begin) + UPD_BLOCK - 1) / UPD_BLOCK), dim3(UPD_BLOCK), 0, nullptr, s, by_level,
                       begin, end);
  }
  UPD_TRY(hipGetLastError());
  return bvh_device_gather_leaf(s.tri_geom, s.bvh_tri, s.n_tri, s.tri_geom_leaf);
}

hipError_t scene_tree_cost(const double *nodes, uint32_t n_nodes, double *ws, double *cost)
{
  if (!cost)
    return hipErrorInvalidValue;
  *cost = 0.0;
  if (n_nodes == 0)
    return hipSuccess;
  if (!nodes)
    return hipErrorInvalidValue;
  /* level l's sums go to buf[l & 1]: the first holds a sum per block of nodes, the second a sum per block of those; every later
   * level is shorter than the one two before it */
  const uint32_t b1 = (n_nodes + BVH_COST_BLOCK - 1) / BVH_COST_BLOCK;
  hipError_t e = hipSuccess;
  double *own = nullptr;
  if (!ws)
  {
    e = hipMalloc(&own, scene_tree_cost_ws_doubles(n_nodes) * sizeof(double));
    if (e != hipSuccess)
    {
      (void)hipGetLastError();
      return e;
    }
    ws = own;
  }
  double *buf[2] = {ws, ws + b1};
  const double *in = nullptr;
  uint32_t n = n_nodes;
  int k = 0;
  for (;; k ^= 1)
  {
    const uint32_t blocks = (n + BVH_COST_BLOCK - 1) / BVH_COST_BLOCK;
    hipLaunchKernelGGL(k_tree_cost, dim3(blocks), dim3(BVH_COST_BLOCK), 0, nullptr, nodes, n_nodes, in, n, buf[k]);
    if (blocks == 1)
      break;
    in = buf[k];
    n = blocks;
  }
  e = hipGetLastError();
  if (e == hipSuccess)
    e = hipMemcpy(cost, buf[k], sizeof(double), hipMemcpyDeviceToHost);
  if (own)
    (void)hipFree(own);
  return e;
}

/* ---- the sphere half ---- */
namespace
{
hipError_t launch_update_spheres(const double *spheres, uint32_t n, double *entry, double *geom4, unsigned long long *words)
{
  if (words)
  {
    const unsigned long long h[SCENE_SPHERE_WORDS] = {key_of(0.0), key_of(0.0), 0, 0};
    UPD_TRY(hipMemcpy(words, h, sizeof h, hipMemcpyHostToDevice));
  }
  hipLaunchKernelGGL(k_update_spheres, dim3((n + UPD_BLOCK - 1) / UPD_BLOCK), dim3(UPD_BLOCK), 0, nullptr, spheres, n, entry, geom4, words);
  return hipGetLastError();
}
} // namespace

hipError_t scene_update_spheres_check(const double *spheres, uint32_t n, unsigned long long *words, SceneSphereBounds *out, bool *radii_ok)
{
  if (!spheres || !words || !out || !radii_ok || n == 0)
    return hipErrorInvalidValue;
  UPD_TRY(launch_update_spheres(spheres, n, nullptr, nullptr, words));
  unsigned long long h[SCENE_SPHERE_WORDS];
  UPD_TRY(hipMemcpy(h, words, sizeof h, hipMemcpyDeviceToHost));
  *out = SceneSphereBounds();
  out->reach_spheres = double_of(h[0]);
  out->max_center = double_of(h[1]);
  out->wide_range = h[2] ? 1u : 0u;
  *radii_ok = h[3] == 0;
  return hipSuccess;
}

hipError_t scene_update_spheres_write(const double *spheres, uint32_t n, double *entry, double *geom4)
{
  if (!spheres || !entry || !geom4 || n == 0)
    return hipErrorInvalidValue;
  return launch_update_spheres(spheres, n, entry, geom4, nullptr);
}

/* ---- the material half ---- */
namespace
{
hipError_t launch_update_materials(const double *in, const uint32_t *flags, uint32_t n, const double *present, double *material,
                                   double *color_raw, unsigned long long *words)
{
  if (words)
  {
    const unsigned long long h[SCENE_MATERIAL_WORDS] = {key_of(0.0), 0, 0, 0, 0};
    UPD_TRY(hipMemcpy(words, h, sizeof h, hipMemcpyHostToDevice));
  }
  hipLaunchKernelGGL(k_update_materials, dim3((n + UPD_BLOCK - 1) / UPD_BLOCK), dim3(UPD_BLOCK), 0, nullptr, in, flags, n, present,
                     material, color_raw, words);
  return hipGetLastError();
}
} // namespace

hipError_t scene_update_materials_check(const double *in, const uint32_t *flags, uint32_t n, const double *present,
                                        unsigned long long *words, SceneMaterialBounds *out, bool *materials_ok)
{
  if (!in || !present || !words || !out || !materials_ok || n == 0)
    return hipErrorInvalidValue;
  UPD_TRY(launch_update_materials(in, flags, n, present, nullptr, nullptr, words));
  unsigned long long h[SCENE_MATERIAL_WORDS];
  UPD_TRY(hipMemcpy(h, words, sizeof h, hipMemcpyDeviceToHost));
  *out = SceneMaterialBounds();
  out->max_emission = double_of(h[0]);
  out->classes = (h[1] ? SCENE_MATERIAL_REFRACT : 0u) | (h[2] ? SCENE_MATERIAL_CHECKER : 0u) | (h[3] ? SCENE_MATERIAL_MIRROR_GLASS : 0u);
  *materials_ok = h[4] == 0;
  return hipSuccess;
}

hipError_t scene_update_materials_write(const double *in, const uint32_t *flags, uint32_t n, double *material, double *color_raw)
{
  if (!in || !material || !color_raw || n == 0)
    return hipErrorInvalidValue;
  return launch_update_materials(in, flags, n, material, material, color_raw, nullptr);
}

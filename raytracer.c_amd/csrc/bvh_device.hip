/* bvh_device.hip -- the triangle hierarchy built on the device: capped full-sweep SAH over three per-axis sorted lists.
 * The contract is BvhSweep (bvh_build.h): this file computes the same nodes and order, byte for byte, level by level:
 *   boxes + keys      k_boxes                       one thread a triangle (bvh_tri_box, bvh_sort_key)
 *   three sorts       rocprim::radix_sort_pairs     64-bit keys, payload = the index, stable
 *   per level         k_scan<false>, k_carry, k_scan<true>   forward and backward segmented min/max scans of the six box
 *                       components over each list: a wave scan by lane shuffles, the block's waves joined through LDS, the
 *                       blocks' aggregates scanned by one workgroup per (direction, axis), the carry applied on the second
 *                       run; out come the two areas at every position, and the box of every range that was made one level up
 *                     k_cost<0>, k_cost<1>          the arg-min per range, in two integer reductions: the least cost's bits,
 *                       then the least (axis, i) among the positions that have it -- no float atomic decides anything
 *                     k_side, k_flags, rocprim::exclusive_scan, k_scatter   side flags and the stable partition of the lists
 *                     k_refs                        the node records' refs and the next level's node numbers
 *   leaf geometry     k_gather_leaf
 * A range is known to every one of its positions (seg_b, seg_e per position), so no kernel walks a table of ranges and one
 * launch shape serves a range that spans thousands of workgroups and thousands of ranges inside one workgroup alike. */
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <utility>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "bvh_build.h"

namespace
{

constexpr int BVH_BLOCK = 256; /* positions a workgroup: four waves */
constexpr uint32_t BVH_NO_SLOT = 0xFFFFFFFFu;

struct Box
{
  double v[6]; /* lo xyz, hi xyz */
};

__device__ inline Box box_empty()
{
  Box b;
  for (int k = 0; k < 3; k++)
  {
    b.v[k] = HUGE_VAL;
    b.v[3 + k] = -HUGE_VAL;
  }
  return b;
}

__device__ inline Box box_join(const Box &a, const Box &b)
{
  Box r;
  for (int k = 0; k < 3; k++)
  {
    r.v[k] = bvh_min(a.v[k], b.v[k]);
    r.v[3 + k] = bvh_max(a.v[3 + k], b.v[3 + k]);
  }
  return r;
}

__device__ inline Box box_load(const double *p)
{
  Box b;
  for (int k = 0; k < 6; k++)
    b.v[k] = p[k];
  return b;
}

__device__ inline void box_store(double *p, const Box &b)
{
  for (int k = 0; k < 6; k++)
    p[k] = b.v[k];
}

/* Inclusive segmented scan over the workgroup's BVH_BLOCK values in thread order.  f in: this value starts a segment; f out: a
 * segment starts at or before this value inside the workgroup (so what came before the workgroup does not reach it).  Every
 * thread of the workgroup calls it. */
__device__ inline void block_seg_scan(Box &v, bool &f, Box *s_box, uint32_t *s_flag)
{
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int d = 1; d < 64; d <<= 1)
  {
    Box o;
    for (int k = 0; k < 6; k++)
      o.v[k] = __shfl_up(v.v[k], d);
    const int of = __shfl_up((int)f, d);
    if (lane >= d)
    {
      if (!f)
        v = box_join(o, v);
      f = f || of != 0;
    }
  }
  if (lane == 63)
  {
    s_box[wave] = v;
    s_flag[wave] = f;
  }
  __syncthreads();
  Box c = box_empty();
  bool cf = false;
  for (int j = 0; j < wave; j++)
  {
    const bool af = s_flag[j] != 0;
    c = af ? s_box[j] : box_join(c, s_box[j]);
    cf = cf || af;
  }
  if (!f)
    v = box_join(c, v);
  f = f || cf;
  __syncthreads();
}

/* the workspace's arrays, as the kernels see them */
struct BvhWork
{
  uint32_t n, n_blocks;
  const double *box;       /* n x 6 */
  uint32_t *list[2];       /* 3 x n each: the lists of this level, of the next */
  uint32_t *seg_b[2], *seg_e[2]; /* n each: the range [b, e) every position lies in */
  double *agg, *carry;     /* 2 x 3 x n_blocks x 6: a workgroup's trailing segment, what reaches a workgroup from outside */
  uint32_t *agg_flag;      /* 2 x 3 x n_blocks */
  double *area_l, *area_r; /* 3 x n: of the box of [b, p], of [p, e) */
  unsigned long long *best_cost, *best_split; /* n, at a range's b */
  uint32_t *node_of, *slot_of; /* n, at a range's b: its node; its parent's child slot (node * 2 + child) still to be filled */
  uint8_t *side;           /* n, by triangle */
  uint32_t *flags, *sums;  /* 4 n + 1: "goes left" per list and position, then "an inner range starts here" */
  uint32_t *ends;          /* 2: sums[3 n] and sums[4 n], side by side for the level's one read-back */
  double *nodes;
};

__global__ void __launch_bounds__(BVH_BLOCK) k_boxes(const double *tri_geom, uint32_t n, double *box, unsigned long long *keys,
                                                    uint32_t *iota)
{
  const uint32_t t = blockIdx.x * BVH_BLOCK + threadIdx.x;
  if (t >= n)
    return;
  double g[9], b[6], c[3];
  for (int k = 0; k < 9; k++)
    g[k] = tri_geom[9 * (size_t)t + k];
  bvh_tri_box(g, b, c);
  for (int k = 0; k < 6; k++)
    box[6 * (size_t)t + k] = b[k];
  for (int a = 0; a < 3; a++)
    keys[(size_t)a * n + t] = bvh_sort_key(c[a]);
  iota[t] = t;
}

__global__ void __launch_bounds__(BVH_BLOCK) k_root(BvhWork w)
{
  const uint32_t p = blockIdx.x * BVH_BLOCK + threadIdx.x;
  if (p >= w.n)
    return;
  w.seg_b[0][p] = 0;
  w.seg_e[0][p] = w.n;
  if (p == 0)
  {
    w.node_of[0] = 0;
    w.slot_of[0] = BVH_NO_SLOT;
  }
}

/* grid (n_blocks, 3 axes).  FINAL = false: the aggregates of the workgroup's trailing segments.  FINAL = true: with the carries,
 * the areas at every position; on list 0 also the box of a range whose parent still waits for it, and the starting winner. */
template <bool FINAL>
__global__ void __launch_bounds__(BVH_BLOCK) k_scan(BvhWork w)
{
  __shared__ double s_tri[6][BVH_BLOCK]; /* component-major: consecutive lanes, consecutive banks, either way round */
  __shared__ Box s_wave[BVH_BLOCK / 64];
  __shared__ uint32_t s_wflag[BVH_BLOCK / 64];
  const uint32_t axis = blockIdx.y, blk = blockIdx.x, t = threadIdx.x, n = w.n;
  const uint32_t *list = w.list[0] + (size_t)axis * n, *seg_b = w.seg_b[0], *seg_e = w.seg_e[0];
  const uint32_t pf = blk * BVH_BLOCK + t, pb = blk * BVH_BLOCK + (BVH_BLOCK - 1 - t);
  Box v = box_empty();
  uint32_t b = 0, e = 0;
  if (pf < n)
  {
    v = box_load(w.box + 6 * (size_t)list[pf]);
    b = seg_b[pf];
    e = seg_e[pf];
  }
  for (int k = 0; k < 6; k++)
    s_tri[k][t] = v.v[k];
  __syncthreads();
  /* forward: [b, p] */
  bool f = pf < n && pf == b;
  block_seg_scan(v, f, s_wave, s_wflag);
  const size_t fwd = (size_t)axis * w.n_blocks + blk, bwd = (size_t)(3 + axis) * w.n_blocks + blk;
  if (!FINAL)
  {
    if (t == BVH_BLOCK - 1)
    {
      box_store(w.agg + 6 * fwd, v);
      w.agg_flag[fwd] = f;
    }
  }
  else if (pf < n)
  {
    if (!f)
      v = box_join(box_load(w.carry + 6 * fwd), v);
    w.area_l[(size_t)axis * n + pf] = bvh_half_area(v.v, v.v + 3);
    if (axis == 0 && pf == e - 1)
    {
      const uint32_t slot = w.slot_of[b];
      if (slot != BVH_NO_SLOT)
      {
        box_store(w.nodes + (size_t)(slot >> 1) * PT_BVH_SRC_DOUBLES + 6 * (slot & 1u), v);
        w.slot_of[b] = BVH_NO_SLOT;
      }
    }
    if (axis == 0 && pf == b && e - b > PT_BVH_LEAF)
    {
      const double inf = HUGE_VAL;
      unsigned long long bits;
      memcpy(&bits, &inf, sizeof bits);
      w.best_cost[b] = bits;
      w.best_split[b] = ~0ull; /* no candidate yet: winner_of() reads it as the starting winner */
    }
  }
  /* backward: [p, e), the workgroup's positions taken from its last to its first */
  Box u;
  for (int k = 0; k < 6; k++)
    u.v[k] = s_tri[k][BVH_BLOCK - 1 - t];
  bool g = pb < n && pb == seg_e[pb] - 1;
  block_seg_scan(u, g, s_wave, s_wflag);
  if (!FINAL)
  {
    if (t == BVH_BLOCK - 1)
    {
      box_store(w.agg + 6 * bwd, u);
      w.agg_flag[bwd] = g;
    }
  }
  else if (pb < n)
  {
    if (!g)
      u = box_join(box_load(w.carry + 6 * bwd), u);
    w.area_r[(size_t)axis * n + pb] = bvh_half_area(u.v, u.v + 3);
  }
}

/* grid 6 = (direction, axis), one workgroup each: the exclusive segmented scan of the workgroups' aggregates, in the order the
 * direction visits them */
__global__ void __launch_bounds__(BVH_BLOCK) k_carry(BvhWork w)
{
  __shared__ Box s_wave[BVH_BLOCK / 64];
  __shared__ uint32_t s_wflag[BVH_BLOCK / 64];
  __shared__ Box s_run;
  const uint32_t nb = w.n_blocks, t = threadIdx.x;
  const bool backward = blockIdx.x >= 3;
  const size_t base = (size_t)blockIdx.x * nb;
  Box run = box_empty();
  for (uint32_t first = 0; first < nb; first += BVH_BLOCK)
  {
    const uint32_t j = first + t;
    const size_t at = base + (backward ? nb - 1 - j : j);
    Box v = box_empty();
    bool f = false;
    if (j < nb)
    {
      v = box_load(w.agg + 6 * at);
      f = w.agg_flag[at] != 0;
    }
    block_seg_scan(v, f, s_wave, s_wflag);
    if (!f)
      v = box_join(run, v);
    /* what reaches workgroup j + 1 is the inclusive value at j */
    if (j + 1 < nb)
      box_store(w.carry + 6 * (base + (backward ? nb - 2 - j : j + 1)), v);
    if (j == 0)
      box_store(w.carry + 6 * at, box_empty());
    if (t == BVH_BLOCK - 1)
      s_run = v;
    __syncthreads();
    run = s_run;
    __syncthreads();
  }
}

/* the winner of the range [b, e): (axis << 32) | i; the starting winner (axis 0, i = m / 2) where no finite cost replaced it */
__device__ inline unsigned long long winner_of(const BvhWork &w, uint32_t b, uint32_t e)
{
  const unsigned long long s = w.best_split[b];
  return s == ~0ull ? (unsigned long long)((e - b) / 2) : s;
}

/* One unsigned minimum per range, at arr[b]: a wave whose candidates all lie in one range reduces them first. */
__device__ inline void range_min(unsigned long long *arr, uint32_t b, bool valid, unsigned long long key)
{
  const unsigned long long mask = __ballot(valid);
  if (mask == 0)
    return;
  const int first = __ffsll((long long)mask) - 1;
  const uint32_t b0 = __shfl(b, first);
  if (__all(!valid || b == b0))
  {
    unsigned long long k = valid ? key : ~0ull;
    for (int d = 32; d >= 1; d >>= 1)
    {
      const unsigned long long o = __shfl_xor(k, d);
      k = o < k ? o : k;
    }
    if ((int)(threadIdx.x & 63) == first)
      atomicMin(&arr[b0], k);
  }
  else if (valid)
    atomicMin(&arr[b], key);
}

/* grid (n_blocks, 3).  PHASE 0: the least cost of a range; PHASE 1: the least (axis, i) among the positions that have it. */
template <int PHASE>
__global__ void __launch_bounds__(BVH_BLOCK) k_cost(BvhWork w, unsigned long long cap)
{
  const uint32_t axis = blockIdx.y, n = w.n, p = blockIdx.x * BVH_BLOCK + threadIdx.x;
  bool ok = p < n;
  uint32_t b = 0, i = 0;
  unsigned long long bits = 0;
  if (ok)
  {
    b = w.seg_b[0][p];
    const uint32_t m = w.seg_e[0][p] - b;
    i = p - b;
    ok = m > PT_BVH_LEAF && i >= 1 && i <= cap && m - i <= cap;
    if (ok)
    {
      const double cost = bvh_split_cost(w.area_l[(size_t)axis * n + p - 1], i, w.area_r[(size_t)axis * n + p], m) + 0.0;
      ok = cost >= 0.0 && cost < HUGE_VAL; /* an infinite or NaN cost never wins */
      memcpy(&bits, &cost, sizeof bits);
    }
  }
  if (PHASE == 0)
    range_min(w.best_cost, b, ok, bits);
  else
  {
    if (ok)
      ok = bits == w.best_cost[b];
    range_min(w.best_split, b, ok, ((unsigned long long)axis << 32) | i);
  }
}

__global__ void __launch_bounds__(BVH_BLOCK) k_side(BvhWork w)
{
  const uint32_t n = w.n, p = blockIdx.x * BVH_BLOCK + threadIdx.x;
  if (p >= n)
    return;
  const uint32_t b = w.seg_b[0][p], e = w.seg_e[0][p];
  if (e - b <= PT_BVH_LEAF)
    return;
  const unsigned long long split = winner_of(w, b, e);
  const uint32_t axis = (uint32_t)(split >> 32), i = (uint32_t)split;
  w.side[w.list[0][(size_t)axis * n + p]] = p >= b + i;
}

/* grid (n_blocks, 3): the partition's "goes left" flags; on list 0 also the next level's ranges and where its inner ones start */
__global__ void __launch_bounds__(BVH_BLOCK) k_flags(BvhWork w)
{
  const uint32_t axis = blockIdx.y, n = w.n, p = blockIdx.x * BVH_BLOCK + threadIdx.x;
  if (p >= n)
    return;
  const uint32_t b = w.seg_b[0][p], e = w.seg_e[0][p];
  const bool inner = e - b > PT_BVH_LEAF;
  w.flags[(size_t)axis * n + p] = inner && w.side[w.list[0][(size_t)axis * n + p]] == 0;
  if (axis != 0)
    return;
  uint32_t nb = b, ne = e;
  if (inner)
  {
    const uint32_t mid = b + (uint32_t)winner_of(w, b, e);
    if (p < mid)
      ne = mid;
    else
      nb = mid;
  }
  w.seg_b[1][p] = nb;
  w.seg_e[1][p] = ne;
  w.flags[(size_t)3 * n + p] = inner && p == nb && ne - nb > PT_BVH_LEAF;
  if (p == 0)
    w.flags[(size_t)4 * n] = 0;
}

__global__ void __launch_bounds__(BVH_BLOCK) k_scatter(BvhWork w)
{
  const uint32_t axis = blockIdx.y, n = w.n, p = blockIdx.x * BVH_BLOCK + threadIdx.x;
  if (p >= n)
    return;
  const uint32_t b = w.seg_b[0][p], e = w.seg_e[0][p];
  const uint32_t tri = w.list[0][(size_t)axis * n + p];
  uint32_t to = p;
  if (e - b > PT_BVH_LEAF)
  {
    const uint32_t i = (uint32_t)winner_of(w, b, e);
    const uint32_t lefts = w.sums[(size_t)axis * n + p] - w.sums[(size_t)axis * n + b]; /* of [b, p) */
    to = w.side[tri] == 0 ? b + lefts : b + i + (p - b) - lefts;
  }
  w.list[1][(size_t)axis * n + to] = tri;
}

/* the refs of this level's nodes; their children's node numbers and parent slots */
__global__ void __launch_bounds__(BVH_BLOCK) k_refs(BvhWork w, uint32_t next_base)
{
  const uint32_t n = w.n, p = blockIdx.x * BVH_BLOCK + threadIdx.x;
  if (p >= n)
    return;
  if (p == 0)
  {
    w.ends[0] = w.sums[(size_t)3 * n];
    w.ends[1] = w.sums[(size_t)4 * n];
  }
  const uint32_t b = w.seg_b[0][p], e = w.seg_e[0][p];
  if (p != b || e - b <= PT_BVH_LEAF)
    return;
  const uint32_t node = w.node_of[b], mid = b + (uint32_t)winner_of(w, b, e);
  const uint32_t cb[2] = {b, mid}, ce[2] = {mid, e};
  uint32_t refs[2];
  for (int c = 0; c < 2; c++)
  {
    const uint32_t cm = ce[c] - cb[c];
    if (cm <= PT_BVH_LEAF)
      refs[c] = PT_BVH_LEAF_FLAG | (cb[c] << PT_BVH_COUNT_BITS) | cm;
    else
    {
      refs[c] = next_base + (w.sums[(size_t)3 * n + cb[c]] - w.sums[(size_t)3 * n]);
      w.node_of[cb[c]] = refs[c];
    }
    w.slot_of[cb[c]] = node * 2u + (uint32_t)c;
  }
  double *nd = w.nodes + (size_t)node * PT_BVH_SRC_DOUBLES;
  double packed;
  memcpy(&packed, refs, sizeof packed);
  nd[12] = packed;
  for (int k = 13; k < PT_BVH_SRC_DOUBLES; k++)
    nd[k] = 0.0;
}

/* a mesh of one leaf: the root with the leaf and an empty second one (one thread) */
__global__ void k_one_leaf(BvhWork w)
{
  if (blockIdx.x != 0 || threadIdx.x != 0)
    return;
  Box v = box_empty();
  for (uint32_t p = 0; p < w.n; p++)
    v = box_join(v, box_load(w.box + 6 * (size_t)w.list[0][p]));
  box_store(w.nodes, v);
  box_store(w.nodes + 6, v);
  const uint32_t refs[2] = {PT_BVH_LEAF_FLAG | w.n, PT_BVH_LEAF_FLAG};
  double packed;
  memcpy(&packed, refs, sizeof packed);
  w.nodes[12] = packed;
  for (int k = 13; k < PT_BVH_SRC_DOUBLES; k++)
    w.nodes[k] = 0.0;
}

__global__ void __launch_bounds__(BVH_BLOCK) k_gather_leaf(const double *tri_geom, const uint32_t *order, uint32_t n, double *out)
{
  const size_t at = (size_t)blockIdx.x * BVH_BLOCK + threadIdx.x; /* one double a thread */
  if (at >= 9 * (size_t)n)
    return;
  out[at] = tri_geom[9 * (size_t)order[at / 9] + at % 9];
}

struct Events
{
  hipEvent_t ev[2] = {nullptr, nullptr};
  ~Events()
  {
    for (hipEvent_t x : ev)
      if (x)
        (void)hipEventDestroy(x);
  }
};

#define BVH_TRY(expr)           \
  do                            \
  {                             \
    const hipError_t e_ = (expr); \
    if (e_ != hipSuccess)       \
      return e_;                \
  } while (0)

} // namespace

hipError_t bvh_device_build(const double *tri_geom, uint32_t n, BvhDeviceTree *out)
{
  if (!tri_geom || !out || n == 0 || n >= (1u << (31 - PT_BVH_COUNT_BITS)))
    return hipErrorInvalidValue;
  const uint32_t n_blocks = (n + BVH_BLOCK - 1) / BVH_BLOCK;
  int max_depth = 0;
  while (((uint64_t)PT_BVH_LEAF << max_depth) < n)
    max_depth++;

  /* ---- one allocation, carved ---- */
  size_t sort_bytes = 0, scan_bytes = 0;
  BVH_TRY(rocprim::radix_sort_pairs(nullptr, sort_bytes, (unsigned long long *)nullptr, (unsigned long long *)nullptr,
                                    (uint32_t *)nullptr, (uint32_t *)nullptr, (size_t)n, 0u, 64u, (hipStream_t) nullptr));
  BVH_TRY(rocprim::exclusive_scan(nullptr, scan_bytes, (uint32_t *)nullptr, (uint32_t *)nullptr, 0u, (size_t)4 * n + 1,
                                  rocprim::plus<uint32_t>(), (hipStream_t) nullptr));
  size_t total = 0;
  auto carve = [&](size_t bytes) {
    const size_t at = total;
    total += (bytes + 255) & ~(size_t)255;
    return at;
  };
  const size_t N = n, NB = n_blocks;
  const size_t o_box = carve(N * 6 * 8), o_keys = carve(N * 3 * 8), o_keys_out = carve(N * 8), o_iota = carve(N * 4);
  const size_t o_list0 = carve(N * 3 * 4), o_list1 = carve(N * 3 * 4);
  const size_t o_sb0 = carve(N * 4), o_sb1 = carve(N * 4), o_se0 = carve(N * 4), o_se1 = carve(N * 4);
  const size_t o_agg = carve(NB * 36 * 8), o_carry = carve(NB * 36 * 8), o_aggf = carve(NB * 6 * 4);
  const size_t o_al = carve(N * 3 * 8), o_ar = carve(N * 3 * 8);
  const size_t o_bc = carve(N * 8), o_bs = carve(N * 8), o_node = carve(N * 4), o_slot = carve(N * 4), o_side = carve(N);
  const size_t o_flags = carve((N * 4 + 1) * 4), o_sums = carve((N * 4 + 1) * 4), o_ends = carve(8);
  const size_t o_nodes = carve(N * PT_BVH_SRC_DOUBLES * 8); /* inner nodes < leaves <= n */
  const size_t o_tmp = carve(sort_bytes > scan_bytes ? sort_bytes : scan_bytes);
  if (out->workspace)
    (void)hipFree(out->workspace);
  out->workspace = nullptr;
  out->failure = nullptr;
  hipError_t e = hipMalloc(&out->workspace, total);
  if (e != hipSuccess)
  {
    out->workspace = nullptr;
    (void)hipGetLastError();
    return e;
  }
  char *base = static_cast<char *>(out->workspace);
  BvhWork w{};
  w.n = n;
  w.n_blocks = n_blocks;
  double *box = reinterpret_cast<double *>(base + o_box);
  w.box = box;
  w.list[0] = reinterpret_cast<uint32_t *>(base + o_list0);
  w.list[1] = reinterpret_cast<uint32_t *>(base + o_list1);
  w.seg_b[0] = reinterpret_cast<uint32_t *>(base + o_sb0);
  w.seg_b[1] = reinterpret_cast<uint32_t *>(base + o_sb1);
  w.seg_e[0] = reinterpret_cast<uint32_t *>(base + o_se0);
  w.seg_e[1] = reinterpret_cast<uint32_t *>(base + o_se1);
  w.agg = reinterpret_cast<double *>(base + o_agg);
  w.carry = reinterpret_cast<double *>(base + o_carry);
  w.agg_flag = reinterpret_cast<uint32_t *>(base + o_aggf);
  w.area_l = reinterpret_cast<double *>(base + o_al);
  w.area_r = reinterpret_cast<double *>(base + o_ar);
  w.best_cost = reinterpret_cast<unsigned long long *>(base + o_bc);
  w.best_split = reinterpret_cast<unsigned long long *>(base + o_bs);
  w.node_of = reinterpret_cast<uint32_t *>(base + o_node);
  w.slot_of = reinterpret_cast<uint32_t *>(base + o_slot);
  w.side = reinterpret_cast<uint8_t *>(base + o_side);
  w.flags = reinterpret_cast<uint32_t *>(base + o_flags);
  w.sums = reinterpret_cast<uint32_t *>(base + o_sums);
  w.ends = reinterpret_cast<uint32_t *>(base + o_ends);
  w.nodes = reinterpret_cast<double *>(base + o_nodes);
  unsigned long long *keys = reinterpret_cast<unsigned long long *>(base + o_keys);
  unsigned long long *keys_out = reinterpret_cast<unsigned long long *>(base + o_keys_out);
  uint32_t *iota = reinterpret_cast<uint32_t *>(base + o_iota);
  void *tmp = base + o_tmp;

  Events ev;
  BVH_TRY(hipEventCreate(&ev.ev[0]));
  BVH_TRY(hipEventCreate(&ev.ev[1]));
  BVH_TRY(hipEventRecord(ev.ev[0], nullptr));

  const dim3 block(BVH_BLOCK), grid1(n_blocks), grid3(n_blocks, 3);
  hipLaunchKernelGGL(k_boxes, grid1, block, 0, nullptr, tri_geom, n, box, keys, iota);
  for (int a = 0; a < 3; a++)
  {
    size_t bytes = sort_bytes;
    BVH_TRY(rocprim::radix_sort_pairs(tmp, bytes, keys + (size_t)a * n, keys_out, iota, w.list[0] + (size_t)a * n, (size_t)n, 0u, 64u,
                                      (hipStream_t) nullptr));
  }
  uint32_t n_nodes = 0;
  int depth = 0;
  if (n <= PT_BVH_LEAF)
  {
    hipLaunchKernelGGL(k_one_leaf, dim3(1), dim3(64), 0, nullptr, w);
    n_nodes = 1;
    depth = 1;
  }
  else
  {
    hipLaunchKernelGGL(k_root, grid1, block, 0, nullptr, w);
    uint32_t level_base = 0, count = 1;
    for (int level = 0;; level++)
    {
      hipLaunchKernelGGL(k_scan<false>, grid3, block, 0, nullptr, w);
      hipLaunchKernelGGL(k_carry, dim3(6), block, 0, nullptr, w);
      hipLaunchKernelGGL(k_scan<true>, grid3, block, 0, nullptr, w);
      if (count == 0)
        break;
      if (level >= max_depth) /* the cap makes every range of level max_depth a leaf */
      {
        out->failure = "an inner range below the depth cap (the builder's own inconsistency, not a device fault)";
        return hipErrorUnknown;
      }
      depth = level + 1;
      const unsigned long long cap = (unsigned long long)PT_BVH_LEAF << (max_depth - level - 1);
      hipLaunchKernelGGL(k_cost<0>, grid3, block, 0, nullptr, w, cap);
      hipLaunchKernelGGL(k_cost<1>, grid3, block, 0, nullptr, w, cap);
      hipLaunchKernelGGL(k_side, grid1, block, 0, nullptr, w);
      hipLaunchKernelGGL(k_flags, grid3, block, 0, nullptr, w);
      size_t bytes = scan_bytes;
      BVH_TRY(rocprim::exclusive_scan(tmp, bytes, w.flags, w.sums, 0u, (size_t)4 * n + 1, rocprim::plus<uint32_t>(),
                                      (hipStream_t) nullptr));
      hipLaunchKernelGGL(k_scatter, grid3, block, 0, nullptr, w);
      const uint32_t next_base = level_base + count;
      hipLaunchKernelGGL(k_refs, grid1, block, 0, nullptr, w, next_base);
      uint32_t ends[2] = {0, 0}; /* the sums before and after the "inner range starts here" flags: one 8-byte read-back */
      BVH_TRY(hipMemcpy(ends, w.ends, sizeof ends, hipMemcpyDeviceToHost));
      level_base = next_base;
      count = ends[1] - ends[0];
      if ((size_t)level_base + count > N)
      {
        out->failure = "more inner nodes than triangles (the builder's own inconsistency, not a device fault)";
        return hipErrorUnknown;
      }
      std::swap(w.list[0], w.list[1]);
      std::swap(w.seg_b[0], w.seg_b[1]);
      std::swap(w.seg_e[0], w.seg_e[1]);
    }
    n_nodes = level_base;
  }
  BVH_TRY(hipGetLastError());
  BVH_TRY(hipEventRecord(ev.ev[1], nullptr));
  BVH_TRY(hipEventSynchronize(ev.ev[1]));
  BVH_TRY(hipEventElapsedTime(&out->build_ms, ev.ev[0], ev.ev[1]));
  out->nodes = w.nodes;
  out->order = w.list[0];
  out->n_nodes = n_nodes;
  out->depth = depth;
  out->max_depth = max_depth;
  return hipSuccess;
}

hipError_t bvh_device_gather_leaf(const double *tri_geom, const uint32_t *order, uint32_t n, double *tri_geom_leaf)
{
  if (n == 0)
    return hipSuccess;
  const size_t blocks = (9 * (size_t)n + BVH_BLOCK - 1) / BVH_BLOCK;
  hipLaunchKernelGGL(k_gather_leaf, dim3((unsigned)blocks), dim3(BVH_BLOCK), 0, nullptr, tri_geom, order, n, tri_geom_leaf);
  return hipGetLastError();
}

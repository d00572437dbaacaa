/* pt_body_static.h -- the bodies whose lane is (x, sample slice), with fp64 partial sums combined by xor-shuffles:
 *   render_tiles_static  x = a pixel of a tile: pt_render_tiles_v0, the M_REFRACTION fallback kernels, every cast_ray kernel;
 *   trace_sliced         x = an entry of a caller's list, through a front end (pt_kernel.hip: RayFront, PixelFront): the
 *                        radiance-query and the pixel-refinement kernels;
 * and what they share: pend_acquire (the workgroup's slot of the pending-ray pool, its PendStack) and reduce_slices.
 * Part of the one translation unit pt_kernel.hip (included there, in this order: pt_math.h, pt_intersect.h, pt_filter.h,
 * pt_scene_ctx.h, pt_trace.h, pt_body_pooled.h, pt_body_queued.h, pt_body_static.h); device code for gfx950 only. */
#ifndef PT_BODY_STATIC_H
#define PT_BODY_STATIC_H

#define PT_SLICED_ENTRIES (PT_BLOCK / PT_SLICES) /* entries of a caller's list per workgroup (trace_sliced) */

/* ---- what the two bodies share ------------------------------------------------------------------------------------------------ */
/* the four slice sums of a pixel or entry, combined as (S0 + S1) + (S2 + S3) in every one of its four lanes */
__device__ __forceinline__ V3 reduce_slices(V3 acc)
{
  acc.x += __shfl_xor(acc.x, 1);
  acc.y += __shfl_xor(acc.y, 1);
  acc.z += __shfl_xor(acc.z, 1);
  acc.x += __shfl_xor(acc.x, 2);
  acc.y += __shfl_xor(acc.y, 2);
  acc.z += __shfl_xor(acc.z, 2);
  return acc;
}

/* kernels with two-child materials: the workgroup's slot of the pending-ray pool and this lane's PendStack in it.  STACKED false:
 * nothing is taken and the stack holds nothing.  No slot (ok false) is a sizing bug of the pool -- the launchers refuse to launch
 * without one: the workgroup's outputs then come out NaN rather than wrong, and the status word says why (pt_pool_acquire).
 * A barrier stands between thread 0's acquisition and every lane's read of it (STACKED only). */
struct PendSlot
{
  uint32_t slot;
  bool ok;
  PendStack stack;
};
template <bool STACKED>
__device__ __forceinline__ PendSlot pend_acquire(const PtLaunch &L)
{
  __shared__ uint32_t pend_slot_lds;
  if (STACKED)
  {
    if (threadIdx.x == 0)
      pend_slot_lds = pt_pool_acquire(L.pend_flags, L.pend_slots_per_xcd, L.status, PT_FAIL_PEND_SLOT);
    __syncthreads();
  }
  const uint32_t slot = STACKED ? pend_slot_lds : 0u;
  const bool ok = !STACKED || slot != 0xFFFFFFFFu;
  return {slot, ok,
          {STACKED && ok ? L.pend_ws + (size_t)slot * L.pend_slot_doubles + threadIdx.x : nullptr, STACKED && ok ? (int)L.pend_entries : 0,
           PT_BLOCK, PT_PEND_FIELDS * PT_BLOCK}};
}

/* ---- static body: lane = (pixel, sample slice), fp64 partial sums ------------------------
 * Lane l of wave w: pixel (l >> 2) of the wave's 16, sample slice (l & 3): samples s = slice,
 * slice + 4, ...; the four slice sums of a pixel are combined by xor-shuffles in a fixed
 * order.  Floating-point sums have no range limit, which is what scenes with M_REFRACTION
 * need (see render_tiles_pooled); VARIANT 0 of it is the plain reference kernel
 * (RT_HIP_KERNEL_VARIANT=0 of the development build, librt_hip_dev.so). */
/* WHITTED: 0 = trace_path, 1 = cast_ray for scenes where no material has both M_REFLECTION and
 * M_REFRACTION (one child per hit at most: no pending-ray stack), 2 = cast_ray with the stack */
template <int VARIANT, bool REFRACT, bool CHECKER, bool TRIS, bool FILT_LDS, int WHITTED, bool GEOM_LDS>
__device__ __forceinline__ void render_tiles_static(const PtLaunch &L, const bool LIST)
{
  extern __shared__ __attribute__((aligned(16))) double lds[];
  __shared__ float out_f[PT_TILE_PIXELS * 3];
  __shared__ uint8_t out_b[PT_TILE_PIXELS * 3 + 64];
  __shared__ unsigned long long wg_stats[2];

  SceneCtx S_init = stage_scene<GEOM_LDS, FILT_LDS>(L, lds);
  __shared__ double atan_tab[(CHECKER || WHITTED) ? PT_ATAN_TAB : 1];
  if (CHECKER || WHITTED)
  {
    atan_table_to_lds(atan_tab);
    S_init.atan_tab = atan_tab;
  }
  /* the leading wall-sized spheres pruned among themselves before the exact tests (BigPrune: the sign-form kernels of sphere
   * scenes), as in the pooled body -- round 4: the static kernels had gone without */
  __shared__ __attribute__((aligned(16))) float big_tab[12];
  if (WHITTED && FILT_LDS && !TRIS && L.big_pairs != 0u) /* (cast_ray only: in the static M_REFRACTION kernel -- a fallback now -- it costs 8 bytes of scratch at four waves) */
  {
    if (threadIdx.x < 2 + 2 * PT_BIG_PAIRS)
      big_tab[threadIdx.x] = threadIdx.x == 0 ? L.big_delta : (threadIdx.x == 1 ? L.big_tmin : L.big_qmin[threadIdx.x - 2]);
    S_init.big = BigPrune{big_tab, L.big_pairs};
  }
  const SceneCtx S = S_init;
  if (threadIdx.x < 2)
    wg_stats[threadIdx.x] = 0;
  __syncthreads();

  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t pix_in_tile = wave * 16u + (lane >> 2);
  const uint32_t slice = lane & (PT_SLICES - 1);
  const uint32_t slot = launch_slot(L, blockIdx.x, LIST);
  const uint32_t tile = L.tile_first + slot * L.tile_stride;
  const uint32_t px = (tile % L.tiles_x) * PT_TILE + (pix_in_tile & 7u);
  const uint32_t py = (tile / L.tiles_x) * PT_TILE + (pix_in_tile >> 3);
  const bool inside = px < (uint32_t)L.width && py < (uint32_t)L.height;
  const uint32_t pixel = py * (uint32_t)L.width + px;
  const uint32_t spp = (uint32_t)L.samples;
  const CameraRegs cam = load_camera(L);
  /* this launch's samples: [sample_first, s_end), absolute; the lane's are those of its slice, s == slice (mod 4) */
  const uint32_t s_end = L.sample_first + spp;
  const bool keep = L.acc_keep != 0u;
  double *const keep_sum = keep ? L.slice_ws + (size_t)slot * (3u * PT_BLOCK) + threadIdx.x : nullptr;

  V3 acc = {0, 0, 0}; /* sum of finished samples of this lane's slice */
  /* Accumulation (acc_keep): the slice sum goes on from where the previous pass left it, and below it is stored back unreduced.
   * A lane adds the same samples in the same ascending order, one fp64 addition each, whether they come in one launch or in
   * passes: the store and reload between passes keep the double exactly, so every addition has the same operands as in a
   * one-shot launch and pt_resolve_slices, reducing the four slices by the same shuffles, gives the same pixel bit for bit. */
  if (keep)
  {
    acc.x = keep_sum[0];
    acc.y = keep_sum[PT_BLOCK];
    acc.z = keep_sum[2 * PT_BLOCK];
  }
  Path P;
  P.o = {0, 0, 0};
  P.d = {0, 0, 1};
  P.T = {1, 1, 1};
  P.Ls = {0, 0, 0};
  P.rng = 1;
  P.depth = 0;
  uint32_t n_rays = 0, n_casts = 0;
  uint32_t s = inside ? L.sample_first + ((slice - L.sample_first) & (PT_SLICES - 1)) : s_end;
  bool fresh = true;
  /* pend_acquire<STACKED>, written out (the call moves pt_whitted_tiles[_big|_tri|_tri_big][_list]).  Without a slot the tile comes
   * out NaN, bytes 255: see the epilogue */
  constexpr bool STACKED = REFRACT || WHITTED == 2;
  __shared__ uint32_t pend_slot_lds;
  if (STACKED)
  {
    if (threadIdx.x == 0)
      pend_slot_lds = pt_pool_acquire(L.pend_flags, L.pend_slots_per_xcd, L.status, PT_FAIL_PEND_SLOT);
    __syncthreads();
  }
  const uint32_t pend_slot = STACKED ? pend_slot_lds : 0u;
  const bool pend_ok = !STACKED || pend_slot != 0xFFFFFFFFu;
  const PendStack stack = {STACKED && pend_ok ? L.pend_ws + (size_t)pend_slot * L.pend_slot_doubles + threadIdx.x : nullptr,
                           STACKED && pend_ok ? (int)L.pend_entries : 0, PT_BLOCK, PT_PEND_FIELDS * PT_BLOCK};
  if (!pend_ok)
    s = s_end;
  int stack_n = 0;
  unsigned long long *diag_ptr = L.stats;
  (void)diag_ptr;

  while (s < s_end)
  {
    DIAG(0, 1);
    DIAG_LANES(1);
    if (fresh)
    {
      DIAG(6, 1);
      DIAG_LANES(7);
      start_sample(P, cam, rt_rng_pixel_key(L.seed, pixel), px, py, sample_term((uint32_t)s));
      fresh = false;
    }
    n_rays++;
    const bool finished = WHITTED ? whitted_step<TRIS, FILT_LDS, WHITTED == 2>(S, P, n_casts, diag_ptr, stack, stack_n)
                                  : trace_step<VARIANT, REFRACT, CHECKER, TRIS, FILT_LDS>(S, P, n_casts, diag_ptr,
                                                                                          stack, stack_n);
    if (finished)
    {
      acc = v_add(acc, P.Ls);
      s += PT_SLICES;
      fresh = true;
    }
  }

  if (keep)
  { /* a pass of an accumulation: the slice sums stay unreduced (a workgroup without its pool slot makes them NaN for good) */
    const double quiet_nan = __longlong_as_double(0x7FF8000000000000ll);
    keep_sum[0] = pend_ok ? acc.x : quiet_nan;
    keep_sum[PT_BLOCK] = pend_ok ? acc.y : quiet_nan;
    keep_sum[2 * PT_BLOCK] = pend_ok ? acc.z : quiet_nan;
    if (n_rays)
    {
      atomicAdd(&wg_stats[0], (unsigned long long)n_rays);
      atomicAdd(&wg_stats[1], (unsigned long long)n_casts);
    }
    __syncthreads();
    store_tile(L, out_f, out_b, wg_stats, tile, slot, S.n_sph + S.n_tri, false, true);
    if (STACKED && pend_ok && threadIdx.x == 0)
      atomicExch(&L.pend_flags[pend_slot], 0u);
    return;
  }
  /* per-pixel mean: fixed-order reduction over the 4 slice lanes (pt_resolve_slices repeats it) */
  V3 mean = v_scale(reduce_slices(acc), 1.0 / (double)spp); /* :215 */
  if (!pend_ok)
    mean.x = mean.y = mean.z = __longlong_as_double(0x7FF8000000000000ll);
  if (slice == 0)
  {
    out_f[3 * pix_in_tile + 0] = inside ? (float)mean.x : 0.f;
    out_f[3 * pix_in_tile + 1] = inside ? (float)mean.y : 0.f;
    out_f[3 * pix_in_tile + 2] = inside ? (float)mean.z : 0.f;
    out_b[3 * pix_in_tile + 0] = inside ? tonemap(mean.x) : 0;
    out_b[3 * pix_in_tile + 1] = inside ? tonemap(mean.y) : 0;
    out_b[3 * pix_in_tile + 2] = inside ? tonemap(mean.z) : 0;
  }
  if (n_rays)
  {
    atomicAdd(&wg_stats[0], (unsigned long long)n_rays);
    atomicAdd(&wg_stats[1], (unsigned long long)n_casts);
  }
  __syncthreads();
  store_tile(L, out_f, out_b, wg_stats, tile, slot, S.n_sph + S.n_tri, true, true);
  if (STACKED && pend_ok && threadIdx.x == 0)
    atomicExch(&L.pend_flags[pend_slot], 0u); /* every lane is past its last pop (the barrier above) */
}

/* ---- sliced body: a lane = (entry, sample slice), a workgroup = 64 consecutive entries x 4 slices ------------------------------
 * rt_hip.h has the contracts (rt_hip_trace_rays, rt_hip_trace_pixels).  render_tiles_static's loop over a caller's list: entry
 * blockIdx.x * 64 + (threadIdx.x >> 2), slice threadIdx.x & 3; no tiles, `inside` is i < n; fp64 outputs, per-sample values and
 * per-entry counters instead of a float image.  A lane adds its slice's samples k = slice, slice + 4, ... in ascending order to a
 * sum that starts at +0.0; the four slice sums are combined as (S0 + S1) + (S2 + S3) and scaled by 1.0 / (double)S.  BigPrune and
 * the hull-facet rule are off, as in the static trace_path members (MODE 0 without DEFER_DIR reads no `leaving`).
 * What an entry IS belongs to the front end (pt_kernel.hip has the two):
 *   Front::Args                      the kernel's second argument; n, status, radiance, samples, paths, casts are read here
 *   Front::Entry, Front::entry(..)   whether entry i is valid, and whatever the other hooks need of it; LDS of the front end's own
 *                                    is declared in its functions, so only its kernels have it
 *   Front::stream(..)                the index of the entry's stream (seed, index, sample)
 *   Front::fresh(..)                 the Path at the start of the entry's sample k
 *   Front::RULE_SWITCH, no_rules(..) trace_step's option of that name: whether this call's scan runs without the conservative rules
 *   Front::store_extra(..)           further outputs of slice 0
 * entry and fresh fill a local of this body through a reference, as caller_ray and start_sample always did: returned by value, the
 * Entry and the Path moved all ten listings (docs/HISTORY.md). */
template <class Front, bool REFRACT, bool CHECKER, bool TRIS = false, bool FILT_LDS = true, bool GEOM_LDS = true>
__device__ __forceinline__ void trace_sliced(const PtLaunch &L, const typename Front::Args &Q)
{
  static_assert(GEOM_LDS || !FILT_LDS, "a staged filter table comes with staged geometry");
  extern __shared__ __attribute__((aligned(16))) double lds[];
  __shared__ unsigned long long wg_stats[3];
  SceneCtx S_init = stage_scene<GEOM_LDS, FILT_LDS>(L, lds);
  __shared__ double atan_tab[CHECKER ? PT_ATAN_TAB : 1];
  if (CHECKER)
  {
    atan_table_to_lds(atan_tab);
    S_init.atan_tab = atan_tab;
  }
  const SceneCtx S = S_init;
  if (threadIdx.x < 3)
    wg_stats[threadIdx.x] = 0;

  const uint32_t slice = threadIdx.x & (PT_SLICES - 1), entry_in_wg = threadIdx.x / PT_SLICES;
  const uint64_t i = (uint64_t)blockIdx.x * PT_SLICED_ENTRIES + entry_in_wg;
  const bool inside = i < Q.n;
  typename Front::Entry E;
  Front::entry(E, L, Q, i, inside, slice, entry_in_wg);
  const bool valid = E.valid;
  /* the workgroup's slot of the pending-ray pool; the barrier in it also stands between the stores above (wg_stats, the front
   * end's LDS) and their readers */
  const PendSlot pend = pend_acquire<REFRACT>(L);
  if (!REFRACT)
    __syncthreads();
  const uint32_t pend_slot = pend.slot;
  const bool pend_ok = pend.ok;
  const PendStack stack = pend.stack;

  const uint32_t spp = (uint32_t)L.samples;
  const uint64_t pixel_key = rt_rng_pixel_key(L.seed, Front::stream(Q, E, i));
  V3 acc = {0, 0, 0};
  Path P;
  P.o = {0, 0, 0};
  P.d = {0, 0, 1};
  P.T = {1, 1, 1};
  P.Ls = {0, 0, 0};
  P.rng = 1;
  P.depth = 0;
  uint32_t n_rays = 0, n_casts = 0;
  unsigned long long paths = 0, casts = 0; /* of this lane's finished samples */
  uint32_t k = (valid && pend_ok) ? slice : spp;
  bool fresh = true;
  int stack_n = 0;
  unsigned long long *diag_ptr = L.stats;
  (void)diag_ptr;

  while (k < spp)
  {
    const bool first = fresh;
    if (fresh)
    {
      Front::fresh(P, Q, E, pixel_key, k, entry_in_wg);
      fresh = false;
    }
    n_rays++;
    const bool finished = trace_step<1, REFRACT, CHECKER, TRIS, FILT_LDS, 0, false, false, false, PendStack, Front::RULE_SWITCH>(
        S, P, n_casts, diag_ptr, stack, stack_n, nullptr, nullptr, 
        Front::no_rules(E, first));
    if (finished)
    {
      acc = v_add(acc, P.Ls);
      if (Q.samples)
      {
        double *q = Q.samples + 3u * (i * spp + k);
        q[0] = P.Ls.x; q[1] = P.Ls.y; q[2] = P.Ls.z;
      }
      paths += n_rays;
      casts += n_casts;
      n_rays = n_casts = 0;
      k += PT_SLICES;
      fresh = true;
    }
  }

  const double quiet_nan = __longlong_as_double(0x7FF8000000000000ll);
  if (inside && Q.samples && !(valid && pend_ok)) /* an invalid entry: zeros; a workgroup without its pool slot: NaN (the render's rule) */
    for (uint32_t j = slice; j < spp; j += PT_SLICES)
    {
      double *q = Q.samples + 3u * (i * spp + j);
      q[0] = q[1] = q[2] = valid ? quiet_nan : 0.0;
    }
  /* reduce_slices, written out (the call renames registers in the five pixel kernels) */
  acc.x += __shfl_xor(acc.x, 1);
  acc.y += __shfl_xor(acc.y, 1);
  acc.z += __shfl_xor(acc.z, 1);
  acc.x += __shfl_xor(acc.x, 2);
  acc.y += __shfl_xor(acc.y, 2);
  acc.z += __shfl_xor(acc.z, 2);
  V3 mean = v_scale(acc, 1.0 / (double)spp);
  if (valid && !pend_ok)
    mean.x = mean.y = mean.z = quiet_nan;
  if (paths)
  {
    atomicAdd(&wg_stats[0], paths);
    atomicAdd(&wg_stats[1], casts);
  }
  paths += __shfl_xor(paths, 1);
  casts += __shfl_xor(casts, 1);
  paths += __shfl_xor(paths, 2);
  casts += __shfl_xor(casts, 2);
  if (inside && slice == 0)
  {
    if (valid)
      atomicAdd(&wg_stats[2], 1ull);
    if (Q.status)
      Q.status[i] = valid ? 1u : 2u;
    if (Q.radiance)
    {
      double *q = Q.radiance + 3u * i;
      q[0] = mean.x; q[1] = mean.y; q[2] = mean.z;
    }
    if (Q.paths)
      Q.paths[i] = paths;
    if (Q.casts)
      Q.casts[i] = casts;
    Front::store_extra(Q, i, entry_in_wg);
  }
  __syncthreads();
  if (threadIdx.x == 0)
  {
    if (L.stats)
    {
      const unsigned long long c = wg_stats[1];
      atomicAdd(&L.stats[0], wg_stats[0]);
      atomicAdd(&L.stats[1], c);
      atomicAdd(&L.stats[2], c * (unsigned long long)(S.n_sph + S.n_tri));
      atomicAdd(&L.stats[3], wg_stats[2] * (unsigned long long)spp);
    }
    if (REFRACT && pend_ok)
      atomicExch(&L.pend_flags[pend_slot], 0u); /* every lane is past its last pop (the barrier above) */
  }
}

#endif /* PT_BODY_STATIC_H */

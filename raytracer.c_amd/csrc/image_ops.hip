/* image_ops.hip -- the image-space passes: kernels that see buffers of pixels or of list entries and never a scene, a ray or a
 * PtLaunch.  Each is the arithmetic rt_hip.h states for its entry point, in fp64, unfused (-ffp-contract=off, as every source of
 * the shim), and each came with the feature it serves:
 *   pt_untile, pt_untile_aov                    compact tile-major buffers to row-major images
 *   pt_denoise_prepare[_final], _filter[_final]  the edge-avoiding a-trous denoiser (rt_hip_denoise)
 *   pt_reproject, pt_reproject_points           temporal reprojection (rt_hip_reproject*)
 *   pt_prev_points, pt_prev_points_moved        where each hit point was before an update (rt_hip_prev_points*)
 *   pt_upsample                                 guided upsampling (rt_hip_upsample)
 *   pt_select_count / _scan / _add / _scatter   the ordered compaction of a per-pixel map (rt_hip_select_pixels)
 *   pt_blend_pixels                             traced pixels into the frame (rt_hip_blend_pixels)
 * From the path tracer's headers they take pt_math.h alone: its vectors, tonemap and tile_pixel.  The launchers at the end are the
 * ones pt_device.h declares under "the image-space passes"; the C entry points, their checks and their host forms are
 * rt_hip_shim.hip's.  256 threads a workgroup, no scratch; no kernel waits for another workgroup. */
#include <hip/hip_runtime.h>

#include "pt_device.h"
#include "rt_rng.h"
#include "pt_math.h"

/* Scatter compact tile-major buffers to row-major images: one thread per
 * (pixel-in-tile, tile); consecutive threads read consecutive floats. */
extern "C" __global__ __launch_bounds__(256) void pt_untile(const float *tiles_rgb, const uint8_t *tiles_rgb8,
                                                          int width, int height, uint32_t tiles_x,
                                                          uint32_t tile_first, uint32_t tile_stride,
                                                          uint32_t tile_count, float *image_rgb,
                                                          uint8_t *image_rgb8)
{
  const size_t total = (size_t)tile_count * PT_TILE_PIXELS;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (size_t)gridDim.x * blockDim.x)
  {
    const uint32_t k = (uint32_t)(idx / PT_TILE_PIXELS), pit = (uint32_t)(idx % PT_TILE_PIXELS);
    const uint32_t tile = tile_first + k * tile_stride;
    /* tile_pixel, written out: the call moves pt_untile (though not pt_untile_aov below, which has it) */
    const uint32_t x = (tile % tiles_x) * PT_TILE + (pit & 7u);
    const uint32_t y = (tile / tiles_x) * PT_TILE + (pit >> 3);
    if (x >= (uint32_t)width || y >= (uint32_t)height)
      continue;
    const size_t dst = ((size_t)y * width + x) * 3, src = idx * 3;
    if (image_rgb)
    {
      image_rgb[dst + 0] = tiles_rgb[src + 0];
      image_rgb[dst + 1] = tiles_rgb[src + 1];
      image_rgb[dst + 2] = tiles_rgb[src + 2];
    }
    if (image_rgb8)
    {
      image_rgb8[dst + 0] = tiles_rgb8[src + 0];
      image_rgb8[dst + 1] = tiles_rgb8[src + 1];
      image_rgb8[dst + 2] = tiles_rgb8[src + 2];
    }
  }
}

/* The same for the AOV buffers: 1- or 3-channel 32-bit words (float or uint32 alike), one thread per (pixel-in-tile, tile, word) */
extern "C" __global__ __launch_bounds__(256) void pt_untile_aov(const uint32_t *tiles, int width, int height, uint32_t tiles_x,
                                                              uint32_t tile_first, uint32_t tile_stride, uint32_t tile_count,
                                                              uint32_t channels, uint32_t *image)
{
  const size_t total = (size_t)tile_count * PT_TILE_PIXELS * channels;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x)
  {
    const size_t px = idx / channels;
    const uint32_t c = (uint32_t)(idx - px * channels);
    const uint32_t k = (uint32_t)(px / PT_TILE_PIXELS), pit = (uint32_t)(px % PT_TILE_PIXELS);
    const uint32_t tile = tile_first + k * tile_stride;
    uint32_t x, y;
    if (!tile_pixel(tiles_x, tile, pit, width, height, x, y))
      continue;
    image[((size_t)y * width + x) * channels + c] = tiles[idx];
  }
}

/* ---- the denoiser (rt_hip_denoise): edge-avoiding a-trous wavelet filter guided by the first-hit buffers --------------------
 * rt_hip.h states the arithmetic; this is it, operation for operation, in fp64 (-ffp-contract=off: no fused multiply-add).  A lane
 * is a pixel.  pt_denoise_prepare demodulates and packs the guidance (normal + depth: one 16-B load, hits + object: one 8-B load)
 * and the validity flag (e.w); each pt_denoise_filter launch is one iteration, ping-ponging e[0] / e[1]; the _final forms of both
 * remodulate and tonemap instead of storing the signal (L = 0: prepare_final alone).  The tap loop is unrolled and the same for
 * every lane of a wave: out-of-image taps load a clamped pixel and every skip is a predicate on the accumulation, not a branch. */
__device__ __forceinline__ void denoise_store(const PtDenoise &D, size_t p, float ox, float oy, float oz)
{
  if (D.out_rgb)
  {
    D.out_rgb[3 * p + 0] = ox;
    D.out_rgb[3 * p + 1] = oy;
    D.out_rgb[3 * p + 2] = oz;
  }
  if (D.out_rgb8)
  {
    D.out_rgb8[3 * p + 0] = tonemap((double)ox);
    D.out_rgb8[3 * p + 1] = tonemap((double)oy);
    D.out_rgb8[3 * p + 2] = tonemap((double)oz);
  }
}

/* step 4: out = float(e * (a + eps)) (DEMODULATE) or e; an invalid pixel passes its input colour through */
__device__ __forceinline__ void denoise_finish(const PtDenoise &D, size_t p, bool valid, float ex, float ey, float ez)
{
  constexpr double eps = 1.0 / 1024.0;
  if (!valid)
    denoise_store(D, p, D.rgb[3 * p + 0], D.rgb[3 * p + 1], D.rgb[3 * p + 2]);
  else if (D.demodulate)
    denoise_store(D, p, (float)((double)ex * ((double)D.albedo[3 * p + 0] + eps)), (float)((double)ey * ((double)D.albedo[3 * p + 1] + eps)),
                  (float)((double)ez * ((double)D.albedo[3 * p + 2] + eps)));
  else
    denoise_store(D, p, ex, ey, ez);
}

template <bool FINAL>
__device__ __forceinline__ void denoise_prepare(const PtDenoise &D)
{
  constexpr double eps = 1.0 / 1024.0;
  const size_t n = (size_t)D.width * (size_t)D.height;
  const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n)
    return;
  const float cx = D.rgb[3 * p + 0], cy = D.rgb[3 * p + 1], cz = D.rgb[3 * p + 2];
  const bool valid = isfinite(cx) && isfinite(cy) && isfinite(cz);
  float ex = cx, ey = cy, ez = cz;
  if (D.demodulate)
  {
    ex = (float)((double)cx / ((double)D.albedo[3 * p + 0] + eps));
    ey = (float)((double)cy / ((double)D.albedo[3 * p + 1] + eps));
    ez = (float)((double)cz / ((double)D.albedo[3 * p + 2] + eps));
  }
  if (FINAL)
  {
    denoise_finish(D, p, valid, ex, ey, ez);
    return;
  }
  reinterpret_cast<float4 *>(D.e[0])[p] = make_float4(ex, ey, ez, valid ? 1.f : 0.f);
  reinterpret_cast<float4 *>(D.guide)[p] = make_float4(D.normal[3 * p + 0], D.normal[3 * p + 1], D.normal[3 * p + 2], D.depth[p]);
  reinterpret_cast<uint2 *>(D.hit_obj)[p] = make_uint2(D.hits[p], D.object_edges ? D.object[p] : 0u);
}

/* one iteration: e[src] -> e[src ^ 1] at step s (a workgroup = a 16 x 16 block of pixels, a wave = 16 x 4) */
template <bool FINAL>
__device__ __forceinline__ void denoise_filter(const PtDenoise &D, uint32_t src, int32_t step, double S2)
{
  const uint32_t bx = ((uint32_t)D.width + 15u) / 16u;
  const int32_t x = (int32_t)((blockIdx.x % bx) * 16u + (threadIdx.x & 15u));
  const int32_t y = (int32_t)((blockIdx.x / bx) * 16u + (threadIdx.x >> 4));
  if (x >= D.width || y >= D.height)
    return; /* no barrier follows */
  const size_t p = (size_t)y * (size_t)D.width + (size_t)x;
  const float4 *ein = reinterpret_cast<const float4 *>(D.e[src]);
  const float4 *guide = reinterpret_cast<const float4 *>(D.guide);
  const uint2 *hit_obj = reinterpret_cast<const uint2 *>(D.hit_obj);
  const float4 ep = ein[p];
  if (ep.w == 0.f)
  { /* invalid: never filtered, never a neighbour */
    if (FINAL)
      denoise_finish(D, p, false, 0.f, 0.f, 0.f);
    else
      reinterpret_cast<float4 *>(D.e[src ^ 1u])[p] = ep;
    return;
  }
  const float4 gp = guide[p];
  const uint2 hop = hit_obj[p];
  const bool edges = D.object_edges != 0u;
  const double epx = ep.x, epy = ep.y, epz = ep.z;
  const double npx = gp.x, npy = gp.y, npz = gp.z, zp = gp.w;
  const double Dp = D.sigma_z * zp;
  constexpr double h5[5] = {1.0 / 16, 1.0 / 4, 3.0 / 8, 1.0 / 4, 1.0 / 16};
  double W = 0, Ax = 0, Ay = 0, Az = 0;
  /* a row of five taps at a time: unrolling all 25 would hoist every tap's loads (240 VGPRs, one wave per SIMD) */
#pragma unroll 1
  for (int dy = -2; dy <= 2; dy++)
  {
    const int ady = dy < 0 ? -dy : dy;
    const double hy = ady == 0 ? h5[2] : ady == 1 ? h5[1] : h5[0];
#pragma unroll
    for (int dx = -2; dx <= 2; dx++)
    {
      if (dx == 0 && dy == 0)
      { /* the centre: 9/64, no edge terms */
        const double w = 9.0 / 64.0;
        W += w;
        Ax += w * epx;
        Ay += w * epy;
        Az += w * epz;
        continue;
      }
      const int64_t qx = (int64_t)x + (int64_t)step * dx, qy = (int64_t)y + (int64_t)step * dy;
      const bool inside = qx >= 0 && qx < D.width && qy >= 0 && qy < D.height;
      const size_t q = (size_t)(inside ? qy : y) * (size_t)D.width + (size_t)(inside ? qx : x);
      const float4 eq = ein[q], gq = guide[q];
      const uint2 hoq = hit_obj[q];
      const bool bg_p = hop.x == 0u, bg_q = hoq.x == 0u;
      const bool take = inside && eq.w != 0.f && (!edges || hoq.y == hop.y) && bg_p == bg_q;
      double g = (npx * (double)gq.x + npy * (double)gq.y) + npz * (double)gq.z;
      g = (g > 0) ? g : 0.0;
      double wn = g;
      for (uint32_t i = 0; i < D.k; i++)
        wn = wn * wn;
      const int adx = dx < 0 ? -dx : dx, m = adx > ady ? adx : ady;
      const double Dd = Dp * (double)(step * m);
      double Zn = Dd * Dd;
      const double dz = (double)gq.w - zp;
      double Zd = Zn + dz * dz;
      if (Zd == 0)
        Zn = Zd = 1.0;
      if (bg_p && bg_q)
        wn = Zn = Zd = 1.0;
      const double dex = (double)eq.x - epx, dey = (double)eq.y - epy, dez = (double)eq.z - epz;
      const double dc = (dex * dex + dey * dey) + dez * dez;
      const double w = (((h5[dx + 2] * hy) * wn) * (S2 * Zn)) / ((S2 + dc) * Zd);
      W = take ? W + w : W;
      Ax = take ? Ax + w * (double)eq.x : Ax;
      Ay = take ? Ay + w * (double)eq.y : Ay;
      Az = take ? Az + w * (double)eq.z : Az;
    }
  }
  const float ox = (float)(Ax / W), oy = (float)(Ay / W), oz = (float)(Az / W);
  if (FINAL)
    denoise_finish(D, p, true, ox, oy, oz);
  else
    reinterpret_cast<float4 *>(D.e[src ^ 1u])[p] = make_float4(ox, oy, oz, 1.f);
}

extern "C" __global__ __launch_bounds__(256) void pt_denoise_prepare(const PtDenoise D) { denoise_prepare<false>(D); }
extern "C" __global__ __launch_bounds__(256) void pt_denoise_prepare_final(const PtDenoise D) { denoise_prepare<true>(D); }
extern "C" __global__ __launch_bounds__(256) void pt_denoise_filter(const PtDenoise D, uint32_t src, int32_t step, double S2)
{
  denoise_filter<false>(D, src, step, S2);
}
extern "C" __global__ __launch_bounds__(256) void pt_denoise_filter_final(const PtDenoise D, uint32_t src, int32_t step, double S2)
{
  denoise_filter<true>(D, src, step, S2);
}

/* ---- temporal reprojection (rt_hip_reproject): a frame's history carried across a camera move ------------------------------
 * rt_hip.h states the arithmetic; this is it, operation for operation, in fp64 (-ffp-contract=off; the library's IEEE division and
 * correctly rounded sqrt).  A lane is a pixel, a workgroup a 16 x 16 block as pt_denoise_filter's, no LDS.  The pixel's first-hit
 * point is rebuilt from its depth along the centre ray (get_camera_ray as query_rays forms it, vec3_normalize in its library
 * form: any camera bytes are allowed here), projected into the history's camera by Cramer's rule, and the history is fetched
 * with the four bilinear taps that show the same surface.  The taps are unrolled and the same for every lane that reaches them:
 * an out-of-image tap loads the lane's own pixel under a false predicate and every skip is a predicate on the sums, not an
 * added zero.  The bytes are written under a wave-uniform branch (out_rgb8 null: no tonemap). */
__device__ __forceinline__ void reproject_store(const PtReproject &R, size_t p, float ox, float oy, float oz, float len, float mx, float my)
{
  R.out_rgb[3 * p + 0] = ox;
  R.out_rgb[3 * p + 1] = oy;
  R.out_rgb[3 * p + 2] = oz;
  R.out_len[p] = len;
  if (R.out_motion)
  {
    R.out_motion[2 * p + 0] = mx;
    R.out_motion[2 * p + 1] = my;
  }
  if (R.out_rgb8)
  {
    R.out_rgb8[3 * p + 0] = tonemap((double)ox);
    R.out_rgb8[3 * p + 1] = tonemap((double)oy);
    R.out_rgb8[3 * p + 2] = tonemap((double)oz);
  }
}

/* The body of pt_reproject and pt_reproject_points: one text for steps 1, 2 and 4-7, the point source (step 3 or 3') chosen by
 * POINTS.  It is expanded in the kernels themselves and is not an inlined template like denoise_filter: behind a function
 * boundary the same text compiles pt_reproject to another listing (1,298 changed lines of 4,190, tools/isa_diff.py), and this
 * way it keeps the one its measurements were taken on, line for line. */
#define PT_REPROJECT_BODY(POINTS, prev_points)                                                                                                   \
{                                                                                                                                                  \
  const uint32_t bx = ((uint32_t)R.width + 15u) / 16u;                                                                                             \
  const int32_t x = (int32_t)((blockIdx.x % bx) * 16u + (threadIdx.x & 15u));                                                                      \
  const int32_t y = (int32_t)((blockIdx.x / bx) * 16u + (threadIdx.x >> 4));                                                                       \
  if (x >= R.width || y >= R.height)                                                                                                               \
    return; /* no barrier follows */                                                                                                               \
  const size_t p = (size_t)y * (size_t)R.width + (size_t)x;                                                                                        \
  const float cx = R.rgb[3 * p + 0], cy = R.rgb[3 * p + 1], cz = R.rgb[3 * p + 2];                                                                 \
  const float qnan = __uint_as_float(0x7FC00000u);                                                                                                 \
  const double inf = __longlong_as_double(0x7FF0000000000000ll);                                                                                   \
  /* 1. a colour that is not finite passes through and starts no history */                                                                        \
  if (!(isfinite(cx) && isfinite(cy) && isfinite(cz)))                                                                                             \
  {                                                                                                                                                \
    reproject_store(R, p, cx, cy, cz, 0.f, qnan, qnan);                                                                                            \
    return;                                                                                                                                        \
  }                                                                                                                                                \
  /* 2. nothing to look up: the first frame, a background pixel, a depth that is no distance */                                                    \
  const double zp = (double)R.depth[p];                                                                                                            \
  if (!R.hist_rgb || R.hits[p] == 0u || !(zp > 0 && zp < inf))                                                                                     \
  {                                                                                                                                                \
    reproject_store(R, p, cx, cy, cz, 1.f, qnan, qnan);                                                                                            \
    return;                                                                                                                                        \
  }                                                                                                                                                \
  /* 3. the first-hit point: get_camera_ray (raytracer.c:375-384) through the pixel's centre, then point_at; 3'. (POINTS) the                      \
   * point the caller gives, where this surface point was in the history's frame -- not finite: nothing to look up */                              \
  const double w1 = (double)R.width - 1.0, h1 = (double)R.height - 1.0;                                                                            \
  V3 P;                                                                                                                                            \
  if constexpr (POINTS)                                                                                                                            \
  {                                                                                                                                                \
    P = ld3(prev_points + 3 * p);                                                                                                                  \
    if (!(isfinite(P.x) && isfinite(P.y) && isfinite(P.z)))                                                                                        \
    {                                                                                                                                              \
      reproject_store(R, p, cx, cy, cz, 1.f, qnan, qnan);                                                                                          \
      return;                                                                                                                                      \
    }                                                                                                                                              \
  }                                                                                                                                                \
  else                                                                                                                                             \
  {                                                                                                                                                \
    const double u = ((double)x + 0.5) / w1, v = ((double)y + 0.5) / h1;                                                                           \
    const V3 pos = ld3(R.cam.pos);                                                                                                                 \
    const V3 E = v_add(ld3(R.cam.llc), v_add(v_scale(ld3(R.cam.horizontal), u), v_scale(ld3(R.cam.vertical), v)));                                 \
    const V3 d = v_normalize(v_sub(pos, E));                                                                                                       \
    P = v_add(pos, v_scale(d, zp));                                                                                                                \
  }                                                                                                                                                \
  /* 4. where the history's camera saw it: H' us + V' vs + D / s = R', solved for (us, vs, 1 / s) by Cramer's rule */                              \
  const V3 Hh = ld3(R.hist_cam.horizontal), Vh = ld3(R.hist_cam.vertical), posh = ld3(R.hist_cam.pos);                                             \
  const V3 D = v_sub(P, posh);                                                                                                                     \
  const V3 Rr = v_sub(posh, ld3(R.hist_cam.llc));                                                                                                  \
  const V3 N = v_cross(Vh, D);                                                                                                                     \
  const double det = v_dot(Hh, N);                                                                                                                 \
  const double us = v_dot(Rr, N) / det;                                                                                                            \
  const V3 M = v_cross(D, Hh);                                                                                                                     \
  const double vs = v_dot(Rr, M) / det;                                                                                                            \
  const double k = v_dot(Rr, v_cross(Hh, Vh));                                                                                                     \
  const bool front = (k > 0 && det > 0) || (k < 0 && det < 0);                                                                                     \
  const double fx = us * w1 - 0.5, fy = vs * h1 - 0.5;                                                                                             \
  const bool ok = front && fx > -1.0 && fx < (double)R.width && fy > -1.0 && fy < (double)R.height;                                                \
  if (!ok)                                                                                                                                         \
  {                                                                                                                                                \
    reproject_store(R, p, cx, cy, cz, 1.f, qnan, qnan);                                                                                            \
    return;                                                                                                                                        \
  }                                                                                                                                                \
  const float mx = (float)(fx - (double)x), my = (float)(fy - (double)y);                                                                          \
  /* 5. the four taps (ok: floor(fx) is in [-1, w - 1], floor(fy) in [-1, h - 1] -- the conversions are in range) */                               \
  const double x0d = floor(fx), y0d = floor(fy);                                                                                                   \
  const double a = fx - x0d, b = fy - y0d;                                                                                                         \
  const int32_t x0 = (int32_t)x0d, y0 = (int32_t)y0d;                                                                                              \
  const double zexp = sqrt(v_dot(D, D));                                                                                                           \
  const double ztol = R.depth_tol * zexp;                                                                                                          \
  const double npx = R.normal[3 * p + 0], npy = R.normal[3 * p + 1], npz = R.normal[3 * p + 2];                                                    \
  const uint32_t op = R.object[p];                                                                                                                 \
  double W = 0, Ax = 0, Ay = 0, Az = 0, S = 0;                                                                                                     \
_Pragma("unroll")                                                                                                                                  \
  for (int j = 0; j < 2; j++)                                                                                                                      \
  {                                                                                                                                                \
_Pragma("unroll")                                                                                                                                  \
    for (int i = 0; i < 2; i++)                                                                                                                    \
    {                                                                                                                                              \
      const int32_t qx = x0 + i, qy = y0 + j;                                                                                                      \
      const bool inside = qx >= 0 && qx < R.width && qy >= 0 && qy < R.height;                                                                     \
      const size_t q = inside ? (size_t)qy * (size_t)R.width + (size_t)qx : p;                                                                     \
      const double wt = (i ? a : 1.0 - a) * (j ? b : 1.0 - b);                                                                                     \
      const float hx = R.hist_rgb[3 * q + 0], hy = R.hist_rgb[3 * q + 1], hz = R.hist_rgb[3 * q + 2];                                              \
      const double lq = (double)R.hist_len[q], zq = (double)R.hist_depth[q];                                                                       \
      const double g = (npx * (double)R.hist_normal[3 * q + 0] + npy * (double)R.hist_normal[3 * q + 1]) + npz * (double)R.hist_normal[3 * q + 2]; \
      const bool take = inside && isfinite(hx) && isfinite(hy) && isfinite(hz) && lq >= 1.0 && lq < inf && R.hist_hits[q] > 0u &&                  \
                        R.hist_object[q] == op && g >= R.normal_min && __builtin_fabs(zq - zexp) <= ztol;                                          \
      W = take ? W + wt : W;                                                                                                                       \
      Ax = take ? Ax + wt * (double)hx : Ax;                                                                                                       \
      Ay = take ? Ay + wt * (double)hy : Ay;                                                                                                       \
      Az = take ? Az + wt * (double)hz : Az;                                                                                                       \
      S = take ? S + wt * lq : S;                                                                                                                  \
    }                                                                                                                                              \
  }                                                                                                                                                \
  /* 6. the blend: a running mean of up to max_history frames */                                                                                   \
  if (!(W > 0))                                                                                                                                    \
  {                                                                                                                                                \
    reproject_store(R, p, cx, cy, cz, 1.f, mx, my);                                                                                                \
    return;                                                                                                                                        \
  }                                                                                                                                                \
  const float hcx = (float)(Ax / W), hcy = (float)(Ay / W), hcz = (float)(Az / W);                                                                 \
  double Nn = S / W + 1.0;                                                                                                                         \
  if (Nn > R.max_history)                                                                                                                          \
    Nn = R.max_history;                                                                                                                            \
  const double al = 1.0 / Nn;                                                                                                                      \
  const float ox = (float)((double)hcx + ((double)cx - (double)hcx) * al);                                                                         \
  const float oy = (float)((double)hcy + ((double)cy - (double)hcy) * al);                                                                         \
  const float oz = (float)((double)hcz + ((double)cz - (double)hcz) * al);                                                                         \
  reproject_store(R, p, ox, oy, oz, (float)Nn, mx, my);                                                                                            \
}

extern "C" __global__ __launch_bounds__(256) void pt_reproject(const PtReproject R) PT_REPROJECT_BODY(false, (const double *)nullptr)
/* rt_hip_reproject_points: step 3 replaced by the caller's previous points (3 doubles per pixel); the frame's camera is not read */
extern "C" __global__ __launch_bounds__(256) void pt_reproject_points(const PtReproject R, const double *prev_points) PT_REPROJECT_BODY(true, prev_points)
#undef PT_REPROJECT_BODY

/* ---- where each hit point was before a vertex update (rt_hip_prev_points) ----------------------------------------------------
 * rt_hip.h states the arithmetic; this is it in fp64 (-ffp-contract=off).  A lane is an entry, 256 lanes a workgroup, no LDS.  The
 * status, prim, bary and point loads are coalesced; the triangle's nine doubles are the one gather.  A lane reads its own point
 * before it writes, so out may be the hits' point array. */
extern "C" __global__ __launch_bounds__(256) void pt_prev_points(const PtPrevPoints A)
{
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= A.n)
    return;
  const double qnan = __longlong_as_double(0x7FF8000000000000ll);
  double ox = qnan, oy = qnan, oz = qnan;
  if (A.status[i] == 1u)
  {
    const uint32_t prim = A.prim[i];
    if (prim == 0xFFFFFFFFu)
    { /* a sphere does not move: the point's own words (no arithmetic touches them) */
      ox = A.point[3 * i + 0];
      oy = A.point[3 * i + 1];
      oz = A.point[3 * i + 2];
    }
    else if ((uint64_t)prim < A.n_triangles)
    {
      const double u = A.bary[2 * i + 0], v = A.bary[2 * i + 1];
      const double w0 = (1.0 - u) - v;
      const double *t = A.positions + 9 * (size_t)prim;
      ox = (t[0] * w0 + t[3] * u) + t[6] * v;
      oy = (t[1] * w0 + t[4] * u) + t[7] * v;
      oz = (t[2] * w0 + t[5] * u) + t[8] * v;
    }
  }
  A.out[3 * i + 0] = ox;
  A.out[3 * i + 1] = oy;
  A.out[3 * i + 2] = oz;
}

/* ---- the same after the spheres moved too (rt_hip_prev_points_moved) --------------------------------------------------------------
 * pt_prev_points with one more clause: a hit on sphere `object` rides that sphere's translation and uniform scale, from the
 * current sphere (c, r) to the previous one (c', r'): s = r' / r, out_k = c'_k + (point_k - c_k) * s, fp64, unfused, in that
 * order.  The two sphere records (4 doubles each) are the gather of such a lane.  A kernel of its own, so that pt_prev_points'
 * listing stays what it was. */
extern "C" __global__ __launch_bounds__(256) void pt_prev_points_moved(const PtPrevPointsMoved A)
{
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= A.n)
    return;
  const double qnan = __longlong_as_double(0x7FF8000000000000ll);
  double ox = qnan, oy = qnan, oz = qnan;
  if (A.status[i] == 1u)
  {
    const uint32_t prim = A.prim[i];
    if (prim == 0xFFFFFFFFu)
    {
      const uint32_t obj = A.object[i];
      if (A.spheres_static != 0u)
      { /* no spheres given: none moved, the point's own words (no arithmetic touches them) */
        ox = A.point[3 * i + 0];
        oy = A.point[3 * i + 1];
        oz = A.point[3 * i + 2];
      }
      else if ((uint64_t)obj < A.n_spheres)
      {
        const double *was = A.spheres_prev + 4 * (size_t)obj, *now = A.spheres_cur + 4 * (size_t)obj;
        const double s = was[3] / now[3];
        ox = was[0] + (A.point[3 * i + 0] - now[0]) * s;
        oy = was[1] + (A.point[3 * i + 1] - now[1]) * s;
        oz = was[2] + (A.point[3 * i + 2] - now[2]) * s;
      }
    }
    else if ((uint64_t)prim < A.n_triangles)
    {
      const double u = A.bary[2 * i + 0], v = A.bary[2 * i + 1];
      const double w0 = (1.0 - u) - v;
      const double *t = A.positions + 9 * (size_t)prim;
      ox = (t[0] * w0 + t[3] * u) + t[6] * v;
      oy = (t[1] * w0 + t[4] * u) + t[7] * v;
      oz = (t[2] * w0 + t[5] * u) + t[8] * v;
    }
  }
  A.out[3 * i + 0] = ox;
  A.out[3 * i + 1] = oy;
  A.out[3 * i + 2] = oz;
}

/* ---- guided upsampling (rt_hip_upsample): a full-size frame from a low-resolution render -----------------------------------
 * rt_hip.h states the arithmetic; this is it, operation for operation, in fp64 (-ffp-contract=off; the library's IEEE division).
 * A lane is a pixel of the HIGH frame, a workgroup a 16 x 16 block as pt_reproject's, no LDS.  The pixel's place in the low frame
 * follows from get_camera_ray's (x + r) / (w - 1) mapping alone; the four bilinear taps there are weighted by how well their
 * first-hit buffers match the pixel's own full-resolution ones.  The taps are unrolled and the same for every lane: an
 * out-of-image tap loads a clamped address under a false predicate, and every skip is a predicate on the sums, not an added zero.
 * The plain bilinear sums of the fallback ride along (two more fp64 multiply-adds per channel and tap: the kernel is bound by its
 * loads).  The flags, the bytes and the confidence are wave-uniform branches on kernel arguments. */
extern "C" __global__ __launch_bounds__(256) void pt_upsample(const PtUpsample U)
{
  const uint32_t bx = ((uint32_t)U.width + 15u) / 16u;
  const int32_t x = (int32_t)((blockIdx.x % bx) * 16u + (threadIdx.x & 15u));
  const int32_t y = (int32_t)((blockIdx.x / bx) * 16u + (threadIdx.x >> 4));
  if (x >= U.width || y >= U.height)
    return; /* no barrier follows */
  const size_t p = (size_t)y * (size_t)U.width + (size_t)x;
  constexpr double eps = 1.0 / 1024.0;
  const double inf = __longlong_as_double(0x7FF0000000000000ll);
  const bool demod = U.demodulate != 0u, edges = U.object_edges != 0u;
  /* 1. the place in the low frame: -0.5 < fx < 1.5 wl, so floor(fx) is in [-1, 1.5 * 2^20] -- the conversions are in range */
  const double fx = (((double)x + 0.5) * ((double)U.low_width - 1.0)) / ((double)U.width - 1.0) - 0.5;
  const double fy = (((double)y + 0.5) * ((double)U.low_height - 1.0)) / ((double)U.height - 1.0) - 0.5;
  const double x0d = floor(fx), y0d = floor(fy);
  const double a = fx - x0d, b = fy - y0d;
  const int32_t x0 = (int32_t)x0d, y0 = (int32_t)y0d;
  const double npx = U.normal[3 * p + 0], npy = U.normal[3 * p + 1], npz = U.normal[3 * p + 2];
  const double zp = (double)U.depth[p];
  const bool bg_p = U.hits[p] == 0u;
  const uint32_t op = edges ? U.object[p] : 0u;
  const double Dp = U.sigma_depth * zp;
  const double Zn_p = Dp * Dp;
  double W = 0, Ax = 0, Ay = 0, Az = 0; /* the guided sums */
  double Us = 0, Bx = 0, By = 0, Bz = 0; /* the plain bilinear sums over the usable taps */
  bool any = false;
#pragma unroll
  for (int j = 0; j < 2; j++)
  {
#pragma unroll
    for (int i = 0; i < 2; i++)
    {
      /* 2. the tap, its weight and its (demodulated) colour */
      const int32_t qx = x0 + i, qy = y0 + j;
      const bool inside = qx >= 0 && qx < U.low_width && qy >= 0 && qy < U.low_height;
      const int32_t cx = qx < 0 ? 0 : (qx >= U.low_width ? U.low_width - 1 : qx), cy = qy < 0 ? 0 : (qy >= U.low_height ? U.low_height - 1 : qy);
      const size_t q = (size_t)cy * (size_t)U.low_width + (size_t)cx;
      const double wt = (i ? a : 1.0 - a) * (j ? b : 1.0 - b);
      float ex = U.low_rgb[3 * q + 0], ey = U.low_rgb[3 * q + 1], ez = U.low_rgb[3 * q + 2];
      if (demod)
      {
        ex = (float)((double)ex / ((double)U.low_albedo[3 * q + 0] + eps));
        ey = (float)((double)ey / ((double)U.low_albedo[3 * q + 1] + eps));
        ez = (float)((double)ez / ((double)U.low_albedo[3 * q + 2] + eps));
      }
      const bool usable = inside && wt > 0 && isfinite(ex) && isfinite(ey) && isfinite(ez);
      /* 3. the guide weight: the surface terms first, then what overrides them */
      const bool bg_q = U.low_hits[q] == 0u;
      double d = (npx * (double)U.low_normal[3 * q + 0] + npy * (double)U.low_normal[3 * q + 1]) + npz * (double)U.low_normal[3 * q + 2];
      d = (d > 0) ? d : 0.0;
      double wn = d;
      for (uint32_t k = 0; k < U.normal_power_log2; k++)
        wn = wn * wn;
      double Zn = Zn_p;
      const double dz = (double)U.low_depth[q] - zp;
      double Zd = Zn + dz * dz;
      if (Zd == 0)
        Zn = Zd = 1.0;
      double g = (wn * Zn) / Zd;
      if (edges)
        g = U.low_object[q] != op ? 0.0 : g;
      g = bg_p != bg_q ? 0.0 : g;
      g = bg_p && bg_q ? 1.0 : g;
      const double om = wt * g;
      const bool take = usable && om > 0 && om < inf;
      any = any || usable;
      Us = usable ? Us + wt : Us;
      Bx = usable ? Bx + wt * (double)ex : Bx;
      By = usable ? By + wt * (double)ey : By;
      Bz = usable ? Bz + wt * (double)ez : Bz;
      W = take ? W + om : W;
      Ax = take ? Ax + om * (double)ex : Ax;
      Ay = take ? Ay + om * (double)ey : Ay;
      Az = take ? Az + om * (double)ez : Az;
    }
  }
  /* 4. the blend: guided where a tap matched, plain bilinear where none did, nothing where the low frame had nothing */
  const bool guided = W > 0;
  const double den = guided ? W : Us;
  float ox = (float)((guided ? Ax : Bx) / den), oy = (float)((guided ? Ay : By) / den), oz = (float)((guided ? Az : Bz) / den);
  float conf = guided ? (float)(W / Us) : 0.f;
  if (!guided && !any)
  {
    ox = oy = oz = 0.f;
    conf = -1.f;
  }
  /* 5. the full-resolution albedo back, and the bytes */
  if (demod)
  {
    ox = (float)((double)ox * ((double)U.albedo[3 * p + 0] + eps));
    oy = (float)((double)oy * ((double)U.albedo[3 * p + 1] + eps));
    oz = (float)((double)oz * ((double)U.albedo[3 * p + 2] + eps));
  }
  U.out_rgb[3 * p + 0] = ox;
  U.out_rgb[3 * p + 1] = oy;
  U.out_rgb[3 * p + 2] = oz;
  if (U.out_conf)
    U.out_conf[p] = conf;
  if (U.out_rgb8)
  {
    U.out_rgb8[3 * p + 0] = tonemap((double)ox);
    U.out_rgb8[3 * p + 1] = tonemap((double)oy);
    U.out_rgb8[3 * p + 2] = tonemap((double)oz);
  }
}

/* ---- pixel selection (rt_hip_select_pixels): the ordered compaction of a per-pixel map ---------------------------------------
 * Three kinds of launch, in stream order; no workgroup reads what another workgroup of the SAME launch writes, so nothing waits and
 * the result does not depend on scheduling:
 *   pt_select_count    a workgroup = PT_SELECT_BLOCK consecutive pixels, a lane = a pixel: the wave's ballot of the predicate,
 *                      its popcount, the four waves' counts through LDS -> counts[workgroup];
 *   pt_select_scan     a workgroup = PT_SELECT_SCAN consecutive counts (four per lane): their exclusive scan in place, and the
 *                      workgroup's total -> sums[workgroup].  pt_launch_select runs it level by level -- the sums of one level are
 *                      the next level's counts -- until one workgroup covers a level (three levels reach 2^30 counts; 2^32 - 1
 *                      pixels are 2^24), then pt_select_add adds each level's scanned sums back onto the level below.  The top
 *                      level's one total is the count;
 *   pt_select_scatter  pt_select_count's predicate and ballot again: pixel p goes to offsets[workgroup] + the counts of the waves
 *                      before its own + the popcount of the ballot's bits below its lane -- ascending in p by construction.
 * The predicate is rt_hip.h's, in fp64 on the exactly widened float: (lo <= v && v <= hi), negated under `invert`. */
__device__ __forceinline__ bool select_predicate(const PtSelect &A, uint64_t p)
{
  if (p >= A.n)
    return false;
  const double v = (double)A.values[p];
  const bool in = A.lo <= v && v <= A.hi; /* false for NaN */
  return A.invert ? !in : in;
}

extern "C" __global__ __launch_bounds__(PT_SELECT_BLOCK) void pt_select_count(const PtSelect A, uint32_t *__restrict__ counts)
{
  __shared__ uint32_t wave_count[PT_SELECT_BLOCK / 64u];
  const uint64_t p = (uint64_t)blockIdx.x * PT_SELECT_BLOCK + threadIdx.x;
  const unsigned long long ballot = __ballot(select_predicate(A, p));
  if ((threadIdx.x & 63u) == 0u)
    wave_count[threadIdx.x >> 6] = (uint32_t)__popcll(ballot);
  __syncthreads();
  if (threadIdx.x == 0)
    counts[blockIdx.x] = (wave_count[0] + wave_count[1]) + (wave_count[2] + wave_count[3]);
}

/* exclusive scan of data[0 .. m) in place, PT_SELECT_SCAN values per workgroup; sums[workgroup] = the workgroup's total */
extern "C" __global__ __launch_bounds__(256) void pt_select_scan(uint32_t *__restrict__ data, uint32_t m, uint32_t *__restrict__ sums)
{
  static_assert(PT_SELECT_SCAN == 4u * 256u, "four values per lane");
  __shared__ uint32_t lane_total[256];
  const uint32_t base = blockIdx.x * PT_SELECT_SCAN + 4u * threadIdx.x; /* m <= 2^24: no overflow */
  uint32_t v[4];
#pragma unroll
  for (uint32_t j = 0; j < 4u; j++)
    v[j] = base + j < m ? data[base + j] : 0u;
  lane_total[threadIdx.x] = (v[0] + v[1]) + (v[2] + v[3]);
  __syncthreads();
  /* Hillis-Steele over the 256 lane totals: inclusive, eight steps, two barriers each (read, then write) */
  for (uint32_t d = 1u; d < 256u; d <<= 1)
  {
    const uint32_t add = threadIdx.x >= d ? lane_total[threadIdx.x - d] : 0u;
    __syncthreads();
    lane_total[threadIdx.x] += add;
    __syncthreads();
  }
  uint32_t run = threadIdx.x ? lane_total[threadIdx.x - 1u] : 0u;
#pragma unroll
  for (uint32_t j = 0; j < 4u; j++)
  {
    if (base + j < m)
      data[base + j] = run;
    run += v[j];
  }
  if (threadIdx.x == 255u)
    sums[blockIdx.x] = lane_total[255];
}

/* data[i] += offsets[i / PT_SELECT_SCAN]: a level's scanned sums back onto the level below */
extern "C" __global__ __launch_bounds__(256) void pt_select_add(uint32_t *__restrict__ data, uint32_t m, const uint32_t *__restrict__ offsets)
{
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < m)
    data[i] += offsets[i / PT_SELECT_SCAN];
}

extern "C" __global__ __launch_bounds__(PT_SELECT_BLOCK) void pt_select_scatter(const PtSelect A, const uint32_t *__restrict__ offsets,
                                                                                uint32_t *__restrict__ indices, uint32_t capacity)
{
  __shared__ uint32_t wave_count[PT_SELECT_BLOCK / 64u];
  const uint64_t p = (uint64_t)blockIdx.x * PT_SELECT_BLOCK + threadIdx.x;
  const bool selected = select_predicate(A, p);
  const unsigned long long ballot = __ballot(selected);
  const uint32_t wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63u) == 0u)
    wave_count[wave] = (uint32_t)__popcll(ballot);
  __syncthreads();
  uint32_t at = offsets[blockIdx.x];
  for (uint32_t w = 0; w < wave; w++)
    at += wave_count[w];
  at += __builtin_amdgcn_mbcnt_hi((uint32_t)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ballot, 0u)); /* set bits below this lane */
  if (selected && at < capacity)
    indices[at] = (uint32_t)p;
}

/* ---- the blend (rt_hip_blend_pixels): traced pixels into the frame -------------------------------------------------------------
 * rt_hip.h states the arithmetic; this is it, operation for operation, in fp64.  A lane is an entry of the list; the entries name
 * distinct pixels (with duplicates the lanes race for the pixel: some entry's complete or partial result, nothing out of bounds).
 * `weight` may be `prior` itself: a lane reads its pixel's prior before it writes the pixel's weight, and no other lane has that pixel. */
extern "C" __global__ __launch_bounds__(256) void pt_blend_pixels(const PtBlend B)
{
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= B.n)
    return; /* no barrier follows */
  const uint32_t p = B.pixels[i];
  if (p >= B.n_pixels || B.status[i] != 1u)
    return;
  const double rx = B.radiance[3u * i + 0], ry = B.radiance[3u * i + 1], rz = B.radiance[3u * i + 2];
  const double inf = __longlong_as_double(0x7FF0000000000000ll);
  auto finite = [&](double x) { return __builtin_fabs(x) < inf; }; /* false for NaN */
  if (!(finite(rx) && finite(ry) && finite(rz)))
    return;
  const size_t q = (size_t)p;
  const double wa = B.prior_scale * (B.prior ? (double)B.prior[q] : 1.0);
  const double cx = (double)B.rgb[3 * q + 0], cy = (double)B.rgb[3 * q + 1], cz = (double)B.rgb[3 * q + 2];
  float ox, oy, oz;
  double W;
  if (!(wa > 0) || !finite(wa) || !(finite(cx) && finite(cy) && finite(cz)))
  {
    ox = (float)rx; oy = (float)ry; oz = (float)rz;
    W = B.new_weight;
  }
  else
  {
    W = wa + B.new_weight;
    ox = (float)((cx * wa + rx * B.new_weight) / W);
    oy = (float)((cy * wa + ry * B.new_weight) / W);
    oz = (float)((cz * wa + rz * B.new_weight) / W);
  }
  B.rgb[3 * q + 0] = ox;
  B.rgb[3 * q + 1] = oy;
  B.rgb[3 * q + 2] = oz;
  if (B.rgb8)
  {
    B.rgb8[3 * q + 0] = tonemap((double)ox);
    B.rgb8[3 * q + 1] = tonemap((double)oy);
    B.rgb8[3 * q + 2] = tonemap((double)oz);
  }
  if (B.weight)
    B.weight[q] = (float)W;
}

/* ---- launch wrappers (host side), declared in pt_device.h ----------------------
 * The two grids of this file, each written once: a lane an item in workgroups of 256, and a workgroup a 16 x 16 block of pixels. */
static uint64_t groups_of_256(uint64_t n) { return (n + 255u) / 256u; }
static uint32_t blocks_16x16(int32_t width, int32_t height) { return (((uint32_t)width + 15u) / 16u) * (((uint32_t)height + 15u) / 16u); }

/* workgroups of 256 threads for a grid-stride loop over `total` items: one pass, at most 8192 */
static uint32_t untile_blocks(size_t total) { return (uint32_t)min(groups_of_256(total), (uint64_t)8192); }

hipError_t pt_launch_untile(const float *tiles_rgb, const uint8_t *tiles_rgb8, int width, int height,
                            uint32_t tile_first, uint32_t tile_stride, uint32_t tile_count, float *image_rgb,
                            uint8_t *image_rgb8, hipStream_t stream)
{
  const uint32_t tiles_x = ((uint32_t)width + PT_TILE - 1) / PT_TILE;
  hipLaunchKernelGGL(pt_untile, dim3(untile_blocks((size_t)tile_count * PT_TILE_PIXELS)), dim3(256), 0, stream, tiles_rgb, tiles_rgb8, width, height, tiles_x,
                     tile_first, tile_stride, tile_count, image_rgb, image_rgb8);
  return hipGetLastError();
}

hipError_t pt_launch_untile_aov(const uint32_t *tiles, uint32_t channels, int width, int height, uint32_t tile_first,
                                uint32_t tile_stride, uint32_t tile_count, uint32_t *image, hipStream_t stream)
{
  const uint32_t tiles_x = ((uint32_t)width + PT_TILE - 1) / PT_TILE;
  hipLaunchKernelGGL(pt_untile_aov, dim3(untile_blocks((size_t)tile_count * PT_TILE_PIXELS * channels)), dim3(256), 0, stream, tiles, width, height, tiles_x, tile_first, tile_stride,
                     tile_count, channels, image);
  return hipGetLastError();
}

/* ---- the denoiser's launches (rt_hip_denoise) ------------------------------------------------------------------------------ */
hipError_t pt_launch_denoise(const PtDenoise &args, int iterations, double sigma_color, hipStream_t stream)
{
  const uint32_t blocks_1d = (uint32_t)groups_of_256((size_t)args.width * (size_t)args.height);
  const uint32_t blocks_2d = blocks_16x16(args.width, args.height);
  if (iterations == 0)
  {
    hipLaunchKernelGGL(pt_denoise_prepare_final, dim3(blocks_1d), dim3(256), 0, stream, args);
    return hipGetLastError();
  }
  hipLaunchKernelGGL(pt_denoise_prepare, dim3(blocks_1d), dim3(256), 0, stream, args);
  hipError_t e = hipGetLastError();
  double sigma = sigma_color;
  for (int i = 0; i < iterations && e == hipSuccess; i++, sigma *= 0.5)
  {
    const double S2 = sigma * sigma;
    if (i + 1 == iterations)
      hipLaunchKernelGGL(pt_denoise_filter_final, dim3(blocks_2d), dim3(256), 0, stream, args, (uint32_t)(i & 1), (int32_t)1 << i, S2);
    else
      hipLaunchKernelGGL(pt_denoise_filter, dim3(blocks_2d), dim3(256), 0, stream, args, (uint32_t)(i & 1), (int32_t)1 << i, S2);
    e = hipGetLastError();
  }
  return e;
}

/* ---- the reprojection's launch (rt_hip_reproject) --------------------------------------------------------------------------- */
hipError_t pt_launch_reproject(const PtReproject &args, hipStream_t stream)
{
  hipLaunchKernelGGL(pt_reproject, dim3(blocks_16x16(args.width, args.height)), dim3(256), 0, stream, args);
  return hipGetLastError();
}

hipError_t pt_launch_reproject_points(const PtReproject &args, const double *prev_points, hipStream_t stream)
{
  hipLaunchKernelGGL(pt_reproject_points, dim3(blocks_16x16(args.width, args.height)), dim3(256), 0, stream, args, prev_points);
  return hipGetLastError();
}

/* ---- the previous points' launch (rt_hip_prev_points): n in [1, 2^32) ---------------------------------------------------------- */
hipError_t pt_launch_prev_points(const PtPrevPoints &args, hipStream_t stream)
{
  hipLaunchKernelGGL(pt_prev_points, dim3((uint32_t)groups_of_256(args.n)), dim3(256), 0, stream, args);
  return hipGetLastError();
}

hipError_t pt_launch_prev_points_moved(const PtPrevPointsMoved &args, hipStream_t stream)
{
  hipLaunchKernelGGL(pt_prev_points_moved, dim3((uint32_t)groups_of_256(args.n)), dim3(256), 0, stream, args);
  return hipGetLastError();
}

/* ---- the upsampling's launch (rt_hip_upsample) ------------------------------------------------------------------------------- */
hipError_t pt_launch_upsample(const PtUpsample &args, hipStream_t stream)
{
  hipLaunchKernelGGL(pt_upsample, dim3(blocks_16x16(args.width, args.height)), dim3(256), 0, stream, args);
  return hipGetLastError();
}

/* ---- the compaction's launches (rt_hip_select_pixels) ------------------------------------------------------------------------
 * The workspace: level 0 holds the per-workgroup counts (ceil(n / PT_SELECT_BLOCK) words), level l + 1 the workgroup totals of
 * level l's scan (ceil(m_l / PT_SELECT_SCAN) words), down to a level of one word; every level starts on a 256-byte boundary. */
static size_t select_levels(uint64_t n, uint32_t m[8], size_t off[8], int *levels)
{
  size_t total = 0;
  int l = 0;
  for (uint64_t count = (n + PT_SELECT_BLOCK - 1u) / PT_SELECT_BLOCK; l < 8; count = (count + PT_SELECT_SCAN - 1u) / PT_SELECT_SCAN)
  {
    m[l] = (uint32_t)count;
    off[l] = total;
    total += ((size_t)count * sizeof(uint32_t) + 255u) & ~(size_t)255u;
    l++;
    if (count <= 1u)
      break;
  }
  *levels = l;
  return total;
}

size_t pt_select_workspace_bytes(uint64_t n)
{
  uint32_t m[8];
  size_t off[8];
  int levels;
  return n == 0u || n > 0xFFFFFFFFull ? 0 : select_levels(n, m, off, &levels);
}

hipError_t pt_launch_select(const PtSelect &args, void *workspace, uint32_t *indices, uint32_t capacity, uint32_t *count, hipStream_t stream)
{
  if (args.n == 0u || args.n > 0xFFFFFFFFull || workspace == nullptr || count == nullptr || (capacity != 0u && indices == nullptr))
    return hipErrorInvalidValue;
  uint32_t m[8];
  size_t off[8];
  int levels;
  (void)select_levels(args.n, m, off, &levels);
  auto level = [&](int l) { return reinterpret_cast<uint32_t *>(static_cast<char *>(workspace) + off[l]); };
  hipLaunchKernelGGL(pt_select_count, dim3(m[0]), dim3(PT_SELECT_BLOCK), 0, stream, args, level(0));
  /* down: level l scanned in place, its workgroup totals are level l + 1 (m[l + 1] = the scan's workgroups); the last level is one
   * workgroup, whose one total is the count */
  for (int l = 0; l < levels; l++)
  {
    const uint32_t blocks = (m[l] + PT_SELECT_SCAN - 1u) / PT_SELECT_SCAN;
    hipLaunchKernelGGL(pt_select_scan, dim3(blocks), dim3(256), 0, stream, level(l), m[l], blocks == 1u ? count : level(l + 1));
    if (blocks == 1u)
    {
      levels = l + 1;
      break;
    }
  }
  /* up: each level's scanned totals onto the level below */
  for (int l = levels - 2; l >= 0; l--)
    hipLaunchKernelGGL(pt_select_add, dim3((uint32_t)groups_of_256(m[l])), dim3(256), 0, stream, level(l), m[l], level(l + 1));
  if (capacity != 0u)
    hipLaunchKernelGGL(pt_select_scatter, dim3(m[0]), dim3(PT_SELECT_BLOCK), 0, stream, args, level(0), indices, capacity);
  return hipGetLastError();
}

/* ---- the blend's launch (rt_hip_blend_pixels) --------------------------------------------------------------------------------- */
hipError_t pt_launch_blend(const PtBlend &args, hipStream_t stream)
{
  if (args.n == 0u || args.n > 0xFFFFFFFFull)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(pt_blend_pixels, dim3((uint32_t)groups_of_256(args.n)), dim3(256), 0, stream, args);
  return hipGetLastError();
}

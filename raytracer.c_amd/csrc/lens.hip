/* lens.hip -- the thin-lens camera (rt_hip.h, "thin-lens camera"): a frame with depth of field is made of lens rays, the radiance
 * query that exists (rt_hip_trace_rays, untouched) and a per-pixel sum.  What is new is a pure function of its arguments:
 *   k_lens_rays        one thread a (pixel of a slice, fixed sample): the ray of rt_hip.h's contract, operation for operation --
 *                      jitter from the first two draws of the stream (seed, k, 0), the pinhole direction not normalised, the focus
 *                      point, the lens point by rejection from the stream (lens_seed, k, 0), at most PT_LENS_ROUNDS rounds (the loop
 *                      diverges per lane and is left to); 6 doubles a ray, written by ray_store.h's
 *                      wave-transposed stores (shared with probe.hip).
 *   k_lens_accumulate  one thread a (pixel, channel): sum += radiance; status 2 makes the pixel's sums NaN.  No atomics.
 *   k_lens_resolve     one thread a (pixel, channel): sum * (1.0 / S) -> float, and the byte by pt_math.h's tonemap, the device
 *                      function every resolve of pt_kernel.hip calls.  Row-major.
 * fp64, unfused (-ffp-contract=off, as every source of the shim), IEEE division and sqrt.  256 threads a workgroup, no scratch, no
 * LDS; no kernel waits for another workgroup. */
#include <hip/hip_runtime.h>

#include "pt_device.h"
#include "rt_rng.h"
#include "pt_math.h"
#include "ray_store.h"

namespace
{

constexpr int LENS_BLOCK = 256;

__global__ void __launch_bounds__(LENS_BLOCK) k_lens_rays(const PtLensRays A)
{
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave_first = blockIdx.x * LENS_BLOCK + (threadIdx.x & ~63u);
  if (wave_first >= A.n)
    return; /* (the whole wave) */
  const uint32_t in_wave = min(64u, A.n - wave_first);
  /* a lane beyond the slice computes the slice's last ray again and stores nothing: every lane reaches the shuffles */
  const uint32_t i = wave_first + min(lane, in_wave - 1u);
  const uint32_t p = A.pixel_first + i, k = A.index_first + i;
  const uint32_t x = p % A.width, y = p / A.width;

  /* raytracer.c:203-204 from the first two draws of (seed, k, 0) */
  uint64_t state = rt_rng_seed(A.seed, k, 0u);
  const double r0 = rnd(state), r1 = rnd(state);
  const double u = ((double)x + r0) / A.w_minus_1;
  const double v = ((double)y + r1) / A.h_minus_1;
  /* get_camera_ray (raytracer.c:377-381) without its normalisation */
  const V3 pos = ld3(A.position);
  const V3 d = v_sub(pos, v_add(ld3(A.lower_left_corner), v_add(v_scale(ld3(A.horizontal), u), v_scale(ld3(A.vertical), v))));
  const V3 F = v_add(pos, v_scale(d, A.focus_distance));
  /* the lens point: a stream of its own, so that the path's draws do not move */
  uint64_t lens = rt_rng_seed(A.lens_seed, k, 0u);
  double a = 0.0, b = 0.0;
  for (int round = 0; round < PT_LENS_ROUNDS; round++)
  {
    const double ta = 2.0 * rnd(lens) - 1.0;
    const double tb = 2.0 * rnd(lens) - 1.0;
    if (ta * ta + tb * tb < 1.0)
    {
      a = ta;
      b = tb;
      break;
    }
  }
  const double R = A.aperture_radius;
  const V3 L = v_add(pos, v_add(v_scale(ld3(A.ax), a * R), v_scale(ld3(A.ay), b * R)));
  const V3 dir = v_normalize(v_sub(F, L));

  store_wave_rays(A.rays, wave_first, lane, in_wave, L, dir);
}

__global__ void __launch_bounds__(LENS_BLOCK) k_lens_accumulate(const uint32_t *__restrict__ status, const double *__restrict__ radiance,
                                                                 uint32_t pixel_first, uint32_t n, double *__restrict__ sum)
{
  const uint64_t t = (uint64_t)blockIdx.x * LENS_BLOCK + threadIdx.x;
  if (t >= 3u * (uint64_t)n)
    return;
  double *const s = sum + 3u * (uint64_t)pixel_first + t;
  const double next = *s + radiance[t];
  *s = status[t / 3u] == 2u ? __longlong_as_double(0x7FF8000000000000ll) : next;
}

__global__ void __launch_bounds__(LENS_BLOCK) k_lens_resolve(const double *__restrict__ sum, uint64_t n_values, double inv_samples,
                                                              float *__restrict__ rgb, uint8_t *__restrict__ rgb8)
{
  const uint64_t t = (uint64_t)blockIdx.x * LENS_BLOCK + threadIdx.x;
  if (t >= n_values)
    return;
  const double mean = sum[t] * inv_samples;
  if (rgb)
    rgb[t] = (float)mean;
  if (rgb8)
    rgb8[t] = tonemap(mean);
}

} // namespace

hipError_t lens_launch_rays(const PtLensRays &args, hipStream_t stream)
{
  const uint32_t blocks = (uint32_t)(((uint64_t)args.n + LENS_BLOCK - 1u) / LENS_BLOCK);
  hipLaunchKernelGGL(k_lens_rays, dim3(blocks), dim3(LENS_BLOCK), 0, stream, args);
  return hipGetLastError();
}

hipError_t lens_launch_accumulate(const uint32_t *status, const double *radiance, uint32_t pixel_first, uint32_t n, double *sum,
                                  hipStream_t stream)
{
  const uint32_t blocks = (uint32_t)((3u * (uint64_t)n + LENS_BLOCK - 1u) / LENS_BLOCK);
  hipLaunchKernelGGL(k_lens_accumulate, dim3(blocks), dim3(LENS_BLOCK), 0, stream, status, radiance, pixel_first, n, sum);
  return hipGetLastError();
}

hipError_t lens_launch_resolve(const double *sum, uint64_t n_pixels, int32_t samples, float *rgb, uint8_t *rgb8, hipStream_t stream)
{
  const uint64_t n_values = 3u * n_pixels;
  const uint32_t blocks = (uint32_t)((n_values + LENS_BLOCK - 1u) / LENS_BLOCK);
  hipLaunchKernelGGL(k_lens_resolve, dim3(blocks), dim3(LENS_BLOCK), 0, stream, sum, n_values, 1.0 / (double)samples, rgb, rgb8);
  return hipGetLastError();
}

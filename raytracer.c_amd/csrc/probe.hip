/* probe.hip -- light probes (rt_hip.h, "light probes"): a bake is made of probe rays, the radiance query that exists
 * (rt_hip_trace_rays, untouched) and a per-probe fold.  What is new is a pure function of its arguments:
 *   k_probe_rays        one thread a ray index k = probe * S + sample: the ray of rt_hip.h's contract, operation for operation -- a
 *                       direction by rejection from the stream (probe_seed, k, 0), at most PT_PROBE_ROUNDS rounds (the loop diverges
 *                       per lane and is left to), flipped into the normal's hemisphere and started off the surface for a hemisphere
 *                       probe; 6 doubles a ray, written by ray_store.h's wave-transposed stores (shared with lens.hip).
 *   k_probe_fold        one thread a (probe of the slice, basis, channel): sum = sum + (radiance * w) over the probe's rays in the
 *                       slice, in ascending k; status 2 makes the probe's sums NaN.  No atomics: a sum has one writer.
 *   k_probe_resolve     one thread a value: (sum * (1.0 / S)) * K -> double and float.
 *   k_probe_irradiance  one thread an (entry, channel): the nine terms (A_j * coeff) * w_j(n) added in ascending j.
 * The constants are pt_device.h's.  fp64, unfused (-ffp-contract=off, as every source of the shim), IEEE division and sqrt.  256
 * threads a workgroup, no scratch, no LDS; no kernel waits for another workgroup. */
#include <hip/hip_runtime.h>

#include "pt_device.h"
#include "rt_rng.h"
#include "pt_math.h"
#include "ray_store.h"

namespace
{

constexpr int PROBE_BLOCK = 256;

__device__ __forceinline__ double quiet_nan() { return __longlong_as_double(0x7FF8000000000000ll); }

/* basis j of a sphere probe at the direction (x, y, z): rt_hip.h's w_j, the products in the order written */
__device__ __forceinline__ double sh_basis(uint32_t j, double x, double y, double z)
{
  switch (j)
  {
  case 0u: return PT_PROBE_Y0;
  case 1u: return PT_PROBE_Y1 * y;
  case 2u: return PT_PROBE_Y1 * z;
  case 3u: return PT_PROBE_Y1 * x;
  case 4u: return PT_PROBE_Y2A * (x * y);
  case 5u: return PT_PROBE_Y2A * (y * z);
  case 6u: return PT_PROBE_Y2B * (3.0 * (z * z) - 1.0);
  case 7u: return PT_PROBE_Y2A * (x * z);
  default: return PT_PROBE_Y2C * (x * x - y * y);
  }
}

/* the one basis of a hemisphere probe: the clamped cosine to the normal */
__device__ __forceinline__ double cos_basis(double x, double y, double z, V3 n)
{
  const double c = (x * n.x + y * n.y) + z * n.z;
  return c > 0.0 ? c : 0.0;
}

__global__ void __launch_bounds__(PROBE_BLOCK) k_probe_rays(const PtProbeRays A)
{
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave_first = blockIdx.x * PROBE_BLOCK + (threadIdx.x & ~63u);
  if (wave_first >= A.n)
    return; /* (the whole wave) */
  const uint32_t in_wave = min(64u, A.n - wave_first);
  /* a lane beyond the range computes the range's last ray again and stores nothing: every lane reaches the shuffles */
  const uint64_t k = A.k_first + (wave_first + min(lane, in_wave - 1u));
  const uint64_t probe = k / A.samples;

  /* random_on_unit_sphere (raytracer.c:231-243) from a stream of its own, so that the path's draws do not move */
  uint64_t state = rt_rng_seed(A.probe_seed, (uint32_t)k, 0u);
  V3 d = {0.0, 0.0, 1.0};
  for (int round = 0; round < PT_PROBE_ROUNDS; round++)
  {
    const double r1 = rnd(state), r2 = rnd(state), r3 = rnd(state);
    const double x = r1 * 2.0 + -1.0, y = r2 * 2.0 + -1.0, z = r3 * 2.0 + -1.0;
    const double q = (x * x + y * y) + z * z;
    if (q <= 1.0 && q >= PT_PROBE_Q_MIN)
    {
      const V3 p = {x, y, z};
      d = v_scale(p, 1.0 / sqrt(q));
      break;
    }
  }
  V3 o = ld3(A.positions + 3u * probe);
  if (A.hemisphere)
  { /* random_on_hemisphere (raytracer.c:245-253), and the origin off the surface */
    const V3 n = ld3(A.normals + 3u * probe);
    const double c = (d.x * n.x + d.y * n.y) + d.z * n.z;
    if (c < 0.0)
      d = v_scale(d, -1.0);
    o = v_add(o, v_scale(n, A.bias));
  }
  store_wave_rays(A.rays, wave_first, lane, in_wave, o, d);
}

__global__ void __launch_bounds__(PROBE_BLOCK) k_probe_fold(const PtProbeFold A)
{
  const uint32_t bases = A.hemisphere ? 1u : (uint32_t)PT_PROBE_SH;
  const uint64_t t = (uint64_t)blockIdx.x * PROBE_BLOCK + threadIdx.x;
  if (t >= A.n_probes * (3u * bases))
    return;
  const uint64_t probe = A.probe_first + t / (3u * bases);
  const uint32_t r = (uint32_t)(t % (3u * bases)), j = r / 3u, c = r - 3u * j;
  /* the probe's rays that lie in the slice, as indices into the slice's buffers */
  const uint64_t lo = max(A.k_first, probe * A.samples), hi = min(A.k_first + A.n, (probe + 1u) * A.samples);
  V3 n = {0.0, 0.0, 0.0};
  if (A.hemisphere)
    n = ld3(A.normals + 3u * probe);
  double *const s = A.sum + (probe * bases + j) * 3u + c;
  double sum = *s;
  bool invalid = false;
  for (uint64_t i = lo - A.k_first; i < hi - A.k_first; i++)
  {
    const double x = A.rays[6u * i + 3u], y = A.rays[6u * i + 4u], z = A.rays[6u * i + 5u];
    const double w = A.hemisphere ? cos_basis(x, y, z, n) : sh_basis(j, x, y, z);
    sum = sum + A.radiance[3u * i + c] * w;
    invalid |= A.status[i] == 2u;
  }
  if (invalid)
  {
    sum = quiet_nan();
    if (A.probe_status && r == 0u)
      A.probe_status[probe] = 2u;
  }
  *s = sum;
}

__global__ void __launch_bounds__(PROBE_BLOCK) k_probe_resolve(const double *__restrict__ sum, uint64_t n_values, double inv_samples, double k,
                                                                double *__restrict__ coeff, float *__restrict__ coeff_f)
{
  const uint64_t t = (uint64_t)blockIdx.x * PROBE_BLOCK + threadIdx.x;
  if (t >= n_values)
    return;
  const double v = (sum[t] * inv_samples) * k;
  coeff[t] = v;
  if (coeff_f)
    coeff_f[t] = (float)v;
}

__global__ void __launch_bounds__(PROBE_BLOCK) k_probe_irradiance(const double *__restrict__ coeff, uint64_t n_probes,
                                                                   const uint32_t *__restrict__ index, const double *__restrict__ normals,
                                                                   uint64_t m, double *__restrict__ irradiance)
{
  const uint64_t t = (uint64_t)blockIdx.x * PROBE_BLOCK + threadIdx.x;
  if (t >= 3u * m)
    return;
  const uint64_t e = t / 3u;
  const uint32_t c = (uint32_t)(t - 3u * e);
  const uint64_t probe = index[e];
  double E = quiet_nan();
  if (probe < n_probes)
  {
    const V3 n = ld3(normals + 3u * e);
    const double *const a = coeff + probe * (3u * PT_PROBE_SH) + c;
    E = 0.0;
#pragma unroll
    for (uint32_t j = 0; j < (uint32_t)PT_PROBE_SH; j++)
    {
      const double band = j == 0u ? PT_PROBE_A0 : (j < 4u ? PT_PROBE_A1 : PT_PROBE_A2);
      E = E + (band * a[3u * j]) * sh_basis(j, n.x, n.y, n.z);
    }
  }
  irradiance[t] = E;
}

uint32_t blocks_for(uint64_t threads) { return (uint32_t)((threads + PROBE_BLOCK - 1u) / PROBE_BLOCK); }

} // namespace

hipError_t probe_launch_rays(const PtProbeRays &args, hipStream_t stream)
{
  hipLaunchKernelGGL(k_probe_rays, dim3(blocks_for(args.n)), dim3(PROBE_BLOCK), 0, stream, args);
  return hipGetLastError();
}

hipError_t probe_launch_fold(const PtProbeFold &args, hipStream_t stream)
{
  const uint64_t threads = args.n_probes * 3u * (args.hemisphere ? 1u : (uint32_t)PT_PROBE_SH);
  hipLaunchKernelGGL(k_probe_fold, dim3(blocks_for(threads)), dim3(PROBE_BLOCK), 0, stream, args);
  return hipGetLastError();
}

hipError_t probe_launch_resolve(const double *sum, uint64_t n_values, int32_t samples, double k, double *coeff, float *coeff_f,
                                hipStream_t stream)
{
  hipLaunchKernelGGL(k_probe_resolve, dim3(blocks_for(n_values)), dim3(PROBE_BLOCK), 0, stream, sum, n_values, 1.0 / (double)samples, k, coeff,
                     coeff_f);
  return hipGetLastError();
}

hipError_t probe_launch_irradiance(const double *coeff, uint64_t n_probes, const uint32_t *index, const double *normals, uint64_t m,
                                   double *irradiance, hipStream_t stream)
{
  hipLaunchKernelGGL(k_probe_irradiance, dim3(blocks_for(3u * m)), dim3(PROBE_BLOCK), 0, stream, coeff, n_probes, index, normals, m, irradiance);
  return hipGetLastError();
}

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
 *   k_probe_grid_positions  one thread a probe of a regular grid: origin + (double)i * step per axis.
 *   k_probe_shade       one thread an entry (a point and a normal): the cell, the eight corners' weights, the blend of their 27
 *                       coefficients in registers, the irradiance and the colour (rt_hip.h, "probe grids", operation for operation).
 *                       A wave whose valid lanes share a cell reads the coefficients through wave-uniform loads.
 *   k_probe_pixel_centres, k_probe_emission, k_probe_tonemap  what rt_hip_probe_preview puts around the shade.
 *   k_probe_depth_fold  one thread a (probe of the slice, texel of its octahedral map): the weight and the two depth moments of the
 *                       probe's rays in the slice, in ascending k, from a ray query's status words and t (rt_hip.h, "probe visibility").
 *   k_probe_depth_resolve  one thread a (probe, texel): the mean depth and the mean squared depth.
 *   k_probe_shade_vis   k_probe_shade with a Chebyshev visibility weight a corner, looked up per lane in the probe's map.
 *   k_probe_grid_positions_strided, k_probe_coeff_blend, k_probe_moment_blend, k_probe_age_step  an update round (rt_hip.h, "probe
 *                       updates"): the positions of the round's probes, a round's fresh sums blended into the grid's coefficients and
 *                       moments by each probe's age, the ages stepped.
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

/* ---- probe grids (rt_hip.h, "probe grids") ---- */

/* the position of probe index i on axis a: the product rounded before the add */
__device__ __forceinline__ double grid_at(const PtGrid &G, int a, uint32_t i) { return G.origin[a] + (double)i * G.step[a]; }

__global__ void __launch_bounds__(PROBE_BLOCK) k_probe_grid_positions(const PtGrid G, double *__restrict__ positions)
{
  const uint32_t i = blockIdx.x * PROBE_BLOCK + threadIdx.x;
  if (i >= G.count[0] * G.count[1] * G.count[2])
    return;
  const uint32_t ix = i % G.count[0], r = i / G.count[0], iy = r % G.count[1], iz = r / G.count[1];
  positions[3u * (size_t)i + 0u] = grid_at(G, 0, ix);
  positions[3u * (size_t)i + 1u] = grid_at(G, 1, iy);
  positions[3u * (size_t)i + 2u] = grid_at(G, 2, iz);
}

/* step 2 of the contract on one axis: the lower probe index and the fraction; a NaN coordinate reads cell 0 (the function is total) */
__device__ __forceinline__ uint32_t grid_cell(const PtGrid &G, int a, double p, double &f)
{
  const uint32_t N = G.count[a];
  double g = (p - G.origin[a]) / G.step[a];
  g = g > 0.0 ? g : 0.0;
  const double top = (double)(N - 1u);
  g = g < top ? g : top;
  uint32_t i0 = (uint32_t)g;
  if (N >= 2u && i0 > N - 2u)
    i0 = N - 2u;
  f = g - (double)i0;
  return i0;
}

#ifndef PT_SHADE_UNIFORM
#define PT_SHADE_UNIFORM 1 /* 0: the per-lane gather alone (tools/probe_shade_bench.py's other arm) */
#endif

/* Steps 3 and 4: the eight corners of the cell whose lower probe is (x0, y0, z0), in ascending c.  The caller gives the cell either as
 * each lane's own registers or as the wave's one cell in scalar registers -- then the addresses are wave-uniform and the coefficients
 * come through scalar loads; the operations on B and W, and their order, are the same text. */
__device__ __forceinline__ void shade_blend(const PtProbeShade &A, uint32_t x0, uint32_t y0, uint32_t z0, const double (&wx)[2],
                                            const double (&wy)[2], const double (&wz)[2], V3 p, V3 n, bool valid, double (&B)[27], double &W)
{
  const PtGrid &G = A.grid;
  const uint32_t x1 = G.count[0] >= 2u ? x0 + 1u : 0u, y1 = G.count[1] >= 2u ? y0 + 1u : 0u, z1 = G.count[2] >= 2u ? z0 + 1u : 0u;
#pragma unroll
  for (uint32_t c = 0; c < 8u; c++)
  {
    const uint32_t bx = c & 1u, by = (c >> 1) & 1u, bz = c >> 2;
    const uint32_t ix = bx ? x1 : x0, iy = by ? y1 : y0, iz = bz ? z1 : z0;
    double w = (wx[bx] * wy[by]) * wz[bz];
    if (G.flags & PT_GRID_FACING)
    {
      const V3 v = {grid_at(G, 0, ix) - p.x, grid_at(G, 1, iy) - p.y, grid_at(G, 2, iz) - p.z};
      const double q = (v.x * v.x + v.y * v.y) + v.z * v.z;
      const double cs = q > 0.0 ? ((v.x * n.x + v.y * n.y) + v.z * n.z) * (1.0 / sqrt(q)) : 1.0;
      const double s = (cs + 1.0) * 0.5;
      w = w * (s * s + PT_GRID_FACE_FLOOR);
    }
    if (valid && w != 0.0) /* (a NaN weight does not skip) */
    {
      const double *__restrict__ const a = A.coeff + (size_t)((iz * G.count[1] + iy) * G.count[0] + ix) * (3u * PT_PROBE_SH);
#pragma unroll
      for (uint32_t k = 0; k < 27u; k++)
        B[k] = B[k] + (w * a[k]);
      W = W + w;
    }
  }
}

/* One thread an entry.  A lane beyond m shades entry m - 1 again and stores nothing, so that every lane of a wave reaches the
 * wave-wide test: if the VALID lanes of the wave share one cell, its index goes to scalar registers (the first valid lane's, read
 * across, and a vote that all agree) and shade_blend's loads become wave-uniform; a wave that straddles cells gathers per lane. */
__global__ void __launch_bounds__(PROBE_BLOCK) k_probe_shade(const PtProbeShade A)
{
  const uint32_t t = blockIdx.x * PROBE_BLOCK + threadIdx.x;
  const bool stores = t < A.m;
  const size_t e = stores ? t : A.m - 1u;
  const V3 p = ld3(A.points + 3u * e), n = ld3(A.normals + 3u * e);
  const bool miss = A.status && A.status[e] != 1u;
  /* x - x is +-0.0 for a finite x and NaN for any other */
  const bool finite = ((p.x - p.x) + (p.y - p.y)) + (p.z - p.z) == 0.0 && ((n.x - n.x) + (n.y - n.y)) + (n.z - n.z) == 0.0;
  const bool valid = !miss && finite;

  double fx, fy, fz;
  const uint32_t x0 = grid_cell(A.grid, 0, p.x, fx), y0 = grid_cell(A.grid, 1, p.y, fy), z0 = grid_cell(A.grid, 2, p.z, fz);
  const double wx[2] = {1.0 - fx, fx}, wy[2] = {1.0 - fy, fy}, wz[2] = {1.0 - fz, fz};

  double B[27], W = 0.0;
#pragma unroll
  for (uint32_t k = 0; k < 27u; k++)
    B[k] = 0.0;
#if PT_SHADE_UNIFORM
  const unsigned long long voters = __ballot(valid);
  if (voters != 0ull)
  {
    const int first = __builtin_ctzll(voters);
    const uint32_t ux = __builtin_amdgcn_readfirstlane(__builtin_amdgcn_readlane((int)x0, first)),
                   uy = __builtin_amdgcn_readfirstlane(__builtin_amdgcn_readlane((int)y0, first)),
                   uz = __builtin_amdgcn_readfirstlane(__builtin_amdgcn_readlane((int)z0, first));
    if (__all(!valid || (x0 == ux && y0 == uy && z0 == uz)))
      shade_blend(A, ux, uy, uz, wx, wy, wz, p, n, valid, B, W);
    else
      shade_blend(A, x0, y0, z0, wx, wy, wz, p, n, valid, B, W);
  }
#else
  shade_blend(A, x0, y0, z0, wx, wy, wz, p, n, valid, B, W);
#endif

  /* step 5 */
  double E[3];
#pragma unroll
  for (uint32_t ch = 0; ch < 3u; ch++)
  {
    double s = 0.0;
#pragma unroll
    for (uint32_t j = 0; j < (uint32_t)PT_PROBE_SH; j++)
    {
      const double band = j == 0u ? PT_PROBE_A0 : (j < 4u ? PT_PROBE_A1 : PT_PROBE_A2);
      s = s + (band * B[3u * j + ch]) * sh_basis(j, n.x, n.y, n.z);
    }
    s = s / W;
    E[ch] = s < 0.0 ? 0.0 : s;
  }
  if (!stores)
    return;
  /* steps 6 and 7 */
  if (A.irradiance)
  {
#pragma unroll
    for (uint32_t ch = 0; ch < 3u; ch++)
      A.irradiance[3u * e + ch] = miss ? 0.0 : (valid ? E[ch] : quiet_nan());
  }
  if (A.color)
  {
#pragma unroll
    for (uint32_t ch = 0; ch < 3u; ch++)
    {
      const double add = A.add ? (double)A.add[3u * e + ch] : 0.0;
      const double albedo = (double)(A.albedo ? A.albedo[3u * e + ch] : 1.0f);
      const double lit = ((albedo * E[ch]) * PT_GRID_INV_PI) + add;
      A.color[3u * e + ch] = miss ? (float)((double)A.grid.miss_color[ch] + add) : (valid ? (float)lit : (float)quiet_nan());
    }
  }
}

/* what rt_hip_probe_preview puts around the shade: the pixel centres, the emission of what a pixel's ray hit, the bytes */
__global__ void __launch_bounds__(PROBE_BLOCK) k_probe_pixel_centres(uint32_t width, uint32_t n, double w_minus_1, double h_minus_1,
                                                                      double *__restrict__ uv)
{
  const uint32_t p = blockIdx.x * PROBE_BLOCK + threadIdx.x;
  if (p >= n)
    return;
  const uint32_t y = p / width, x = p - y * width;
  uv[2u * (size_t)p + 0u] = ((double)x + 0.5) / w_minus_1;
  uv[2u * (size_t)p + 1u] = ((double)y + 0.5) / h_minus_1;
}

__global__ void __launch_bounds__(PROBE_BLOCK) k_probe_emission(const uint32_t *__restrict__ object, uint64_t n_values,
                                                                 const double *__restrict__ emission, uint32_t stride, uint32_t n_objects,
                                                                 float *__restrict__ add)
{
  const uint64_t t = (uint64_t)blockIdx.x * PROBE_BLOCK + threadIdx.x;
  if (t >= n_values)
    return;
  const uint64_t i = t / 3u;
  const uint32_t c = (uint32_t)(t - 3u * i), o = object[i];
  add[t] = o < n_objects ? (float)emission[(size_t)stride * o + c] : 0.0f;
}

__global__ void __launch_bounds__(PROBE_BLOCK) k_probe_tonemap(const float *__restrict__ rgb, uint64_t n_values, uint8_t *__restrict__ rgb8)
{
  const uint64_t t = (uint64_t)blockIdx.x * PROBE_BLOCK + threadIdx.x;
  if (t < n_values)
    rgb8[t] = tonemap((double)rgb[t]);
}

/* ---- probe visibility (rt_hip.h, "probe visibility") ---- */

__device__ __forceinline__ double oct_sgn(double v) { return v >= 0.0 ? 1.0 : -1.0; }

/* the centre direction of texel (tx, ty) of an R x R octahedral map */
__device__ __forceinline__ V3 oct_texel_dir(uint32_t R, uint32_t tx, uint32_t ty)
{
  const double a = (((double)tx + 0.5) / (double)R) * 2.0 - 1.0, b = (((double)ty + 0.5) / (double)R) * 2.0 - 1.0;
  const double z = (1.0 - fabs(a)) - fabs(b);
  double x = a, y = b;
  if (z < 0.0)
  {
    x = (1.0 - fabs(b)) * oct_sgn(a);
    y = (1.0 - fabs(a)) * oct_sgn(b);
  }
  const V3 v = {x, y, z};
  return v_scale(v, 1.0 / sqrt((x * x + y * y) + z * z));
}

/* One thread a (probe of the slice, texel): W, M1 and M2 over the probe's rays in the slice, in ascending k.  A sum has one writer,
 * which loads it and stores it: the slices leave no trace in its bits. */
__global__ void __launch_bounds__(PROBE_BLOCK) k_probe_depth_fold(const PtProbeDepthFold A)
{
  const uint32_t R = A.vis.res, texels = R * R;
  const uint64_t t = (uint64_t)blockIdx.x * PROBE_BLOCK + threadIdx.x;
  if (t >= A.n_probes * texels)
    return;
  const uint64_t probe = A.probe_first + t / texels;
  const uint32_t texel = (uint32_t)(t % texels), ty = texel / R, tx = texel - R * ty;
  const V3 e = oct_texel_dir(R, tx, ty);
  const uint64_t lo = max(A.k_first, probe * A.samples), hi = min(A.k_first + A.n, (probe + 1u) * A.samples);
  double *const s = A.sum + (probe * texels + texel) * 3u;
  double W = s[0], M1 = s[1], M2 = s[2];
  bool invalid = false;
  for (uint64_t i = lo - A.k_first; i < hi - A.k_first; i++)
  {
    const double x = A.rays[6u * i + 3u], y = A.rays[6u * i + 4u], z = A.rays[6u * i + 5u];
    double c = (x * e.x + y * e.y) + z * e.z;
    c = c > 0.0 ? c : 0.0;
    double w = c;
    for (uint32_t k = 0; k < A.vis.sharp; k++)
      w = w * w;
    const uint32_t st = A.status[i];
    const double hit = A.t[i];
    const double dist = st == 1u ? (hit < A.vis.d_max ? hit : A.vis.d_max) : A.vis.d_max;
    W = W + w;
    M1 = M1 + w * dist;
    M2 = M2 + w * (dist * dist);
    invalid |= st == 2u;
  }
  if (invalid)
  {
    W = M1 = M2 = quiet_nan();
    if (A.probe_status && texel == 0u)
      A.probe_status[probe] = 2u;
  }
  s[0] = W;
  s[1] = M1;
  s[2] = M2;
}

__global__ void __launch_bounds__(PROBE_BLOCK) k_probe_depth_resolve(const double *__restrict__ sum, uint64_t n_texels, double d_max,
                                                                      double *__restrict__ moments)
{
  const uint64_t t = (uint64_t)blockIdx.x * PROBE_BLOCK + threadIdx.x;
  if (t >= n_texels)
    return;
  const double W = sum[3u * t], M1 = sum[3u * t + 1u], M2 = sum[3u * t + 2u];
  /* (a NaN W is the probe's invalid mark: it must reach the moments, and NaN > 0 would hide it) */
  const bool nan = W != W;
  moments[2u * t] = nan ? W : (W > 0.0 ? M1 / W : d_max);
  moments[2u * t + 1u] = nan ? W : (W > 0.0 ? M2 / W : d_max * d_max);
}

/* a texel index pair continued across the map's edge: first i, then j */
__device__ __forceinline__ uint32_t oct_texel(int R, int i, int j)
{
  if (i < 0 || i > R - 1)
  {
    i = i < 0 ? 0 : R - 1;
    j = R - 1 - j;
  }
  if (j < 0 || j > R - 1)
  {
    j = j < 0 ? 0 : R - 1;
    i = R - 1 - i;
  }
  return (uint32_t)(i + R * j);
}

/* one axis of the sample position: the lower texel (-1 .. R - 1) and the fraction; a NaN reads from -0.5 (the function is total) */
__device__ __forceinline__ int oct_axis(int R, double a, double &f)
{
  double u = (a * 0.5 + 0.5) * (double)R - 0.5;
  u = u >= -0.5 ? u : -0.5;
  const double top = (double)R - 0.5;
  u = u <= top ? u : top;
  const double fl = floor(u);
  f = u - fl;
  return (int)fl;
}

/* the bilinear lookup of a probe's (mean, mean2) at the direction v, |v| > 0 */
__device__ __forceinline__ void oct_lookup(const double *__restrict__ map, uint32_t res, V3 v, double &mean, double &mean2)
{
  const int R = (int)res;
  const double s = (fabs(v.x) + fabs(v.y)) + fabs(v.z);
  double a = v.x / s, b = v.y / s;
  if (v.z < 0.0)
  {
    const double fa = (1.0 - fabs(b)) * oct_sgn(a), fb = (1.0 - fabs(a)) * oct_sgn(b);
    a = fa;
    b = fb;
  }
  double fx, fy;
  const int i0 = oct_axis(R, a, fx), j0 = oct_axis(R, b, fy);
  const double gx = 1.0 - fx, gy = 1.0 - fy;
  const double w00 = gx * gy, w10 = fx * gy, w01 = gx * fy, w11 = fx * fy;
  const double *const m00 = map + 2u * oct_texel(R, i0, j0), *const m10 = map + 2u * oct_texel(R, i0 + 1, j0),
                     *const m01 = map + 2u * oct_texel(R, i0, j0 + 1), *const m11 = map + 2u * oct_texel(R, i0 + 1, j0 + 1);
  mean = ((w00 * m00[0] + w10 * m10[0]) + w01 * m01[0]) + w11 * m11[0];
  mean2 = ((w00 * m00[1] + w10 * m10[1]) + w01 * m01[1]) + w11 * m11[1];
}

/* shade_blend's text with the visibility weight in step 3: a copy, so that k_probe_shade's code does not move.  The cell comes as
 * lanes' registers or as the wave's scalars (the coefficient loads are then wave-uniform); the moment lookups are per lane in both. */
__device__ __forceinline__ void shade_blend_vis(const PtProbeShadeVis &A, uint32_t x0, uint32_t y0, uint32_t z0, const double (&wx)[2],
                                                const double (&wy)[2], const double (&wz)[2], V3 p, V3 n, bool valid, double (&B)[27],
                                                double &W)
{
  const PtGrid &G = A.shade.grid;
  const PtProbeVis &S = A.vis;
  const uint32_t x1 = G.count[0] >= 2u ? x0 + 1u : 0u, y1 = G.count[1] >= 2u ? y0 + 1u : 0u, z1 = G.count[2] >= 2u ? z0 + 1u : 0u;
  const V3 pb = {p.x + n.x * S.bias, p.y + n.y * S.bias, p.z + n.z * S.bias};
#pragma unroll
  for (uint32_t c = 0; c < 8u; c++)
  {
    const uint32_t bx = c & 1u, by = (c >> 1) & 1u, bz = c >> 2;
    const uint32_t ix = bx ? x1 : x0, iy = by ? y1 : y0, iz = bz ? z1 : z0;
    const V3 corner = {grid_at(G, 0, ix), grid_at(G, 1, iy), grid_at(G, 2, iz)};
    double w = (wx[bx] * wy[by]) * wz[bz];
    if (G.flags & PT_GRID_FACING)
    {
      const V3 v = {corner.x - p.x, corner.y - p.y, corner.z - p.z};
      const double q = (v.x * v.x + v.y * v.y) + v.z * v.z;
      const double cs = q > 0.0 ? ((v.x * n.x + v.y * n.y) + v.z * n.z) * (1.0 / sqrt(q)) : 1.0;
      const double s = (cs + 1.0) * 0.5;
      w = w * (s * s + PT_GRID_FACE_FLOOR);
    }
    if (valid && w != 0.0) /* (a NaN weight does not skip) */
    {
      const size_t probe = (size_t)((iz * G.count[1] + iy) * G.count[0] + ix);
      const V3 v = {pb.x - corner.x, pb.y - corner.y, pb.z - corner.z};
      const double q = (v.x * v.x + v.y * v.y) + v.z * v.z;
      const double r = sqrt(q);
      double vis_w = 1.0;
      if (q > 0.0)
      {
        double mean, mean2;
        oct_lookup(A.moments + probe * (2u * S.res * S.res), S.res, v, mean, mean2);
        if (r > mean)
        {
          const double var = fabs(mean * mean - mean2), d = r - mean;
          double ch = var / (var + d * d);
          ch = (ch * ch) * ch;
          vis_w = ch > S.floor ? ch : S.floor;
        }
        if (mean != mean || mean2 != mean2)
          vis_w = quiet_nan();
      }
      w = w * vis_w;
      const double *__restrict__ const a = A.shade.coeff + probe * (3u * PT_PROBE_SH);
#pragma unroll
      for (uint32_t k = 0; k < 27u; k++)
        B[k] = B[k] + (w * a[k]);
      W = W + w;
    }
  }
}

/* k_probe_shade's text around shade_blend_vis */
__global__ void __launch_bounds__(PROBE_BLOCK) k_probe_shade_vis(const PtProbeShadeVis V)
{
  const PtProbeShade &A = V.shade;
  const uint32_t t = blockIdx.x * PROBE_BLOCK + threadIdx.x;
  const bool stores = t < A.m;
  const size_t e = stores ? t : A.m - 1u;
  const V3 p = ld3(A.points + 3u * e), n = ld3(A.normals + 3u * e);
  const bool miss = A.status && A.status[e] != 1u;
  const bool finite = ((p.x - p.x) + (p.y - p.y)) + (p.z - p.z) == 0.0 && ((n.x - n.x) + (n.y - n.y)) + (n.z - n.z) == 0.0;
  const bool valid = !miss && finite;

  double fx, fy, fz;
  const uint32_t x0 = grid_cell(A.grid, 0, p.x, fx), y0 = grid_cell(A.grid, 1, p.y, fy), z0 = grid_cell(A.grid, 2, p.z, fz);
  const double wx[2] = {1.0 - fx, fx}, wy[2] = {1.0 - fy, fy}, wz[2] = {1.0 - fz, fz};

  double B[27], W = 0.0;
#pragma unroll
  for (uint32_t k = 0; k < 27u; k++)
    B[k] = 0.0;
  const unsigned long long voters = __ballot(valid);
  if (voters != 0ull)
  {
    const int first = __builtin_ctzll(voters);
    const uint32_t ux = __builtin_amdgcn_readfirstlane(__builtin_amdgcn_readlane((int)x0, first)),
                   uy = __builtin_amdgcn_readfirstlane(__builtin_amdgcn_readlane((int)y0, first)),
                   uz = __builtin_amdgcn_readfirstlane(__builtin_amdgcn_readlane((int)z0, first));
    if (__all(!valid || (x0 == ux && y0 == uy && z0 == uz)))
      shade_blend_vis(V, ux, uy, uz, wx, wy, wz, p, n, valid, B, W);
    else
      shade_blend_vis(V, x0, y0, z0, wx, wy, wz, p, n, valid, B, W);
  }

  double E[3];
#pragma unroll
  for (uint32_t ch = 0; ch < 3u; ch++)
  {
    double s = 0.0;
#pragma unroll
    for (uint32_t j = 0; j < (uint32_t)PT_PROBE_SH; j++)
    {
      const double band = j == 0u ? PT_PROBE_A0 : (j < 4u ? PT_PROBE_A1 : PT_PROBE_A2);
      s = s + (band * B[3u * j + ch]) * sh_basis(j, n.x, n.y, n.z);
    }
    s = s / W;
    E[ch] = s < 0.0 ? 0.0 : s;
  }
  if (!stores)
    return;
  if (A.irradiance)
  {
#pragma unroll
    for (uint32_t ch = 0; ch < 3u; ch++)
      A.irradiance[3u * e + ch] = miss ? 0.0 : (valid ? E[ch] : quiet_nan());
  }
  if (A.color)
  {
#pragma unroll
    for (uint32_t ch = 0; ch < 3u; ch++)
    {
      const double add = A.add ? (double)A.add[3u * e + ch] : 0.0;
      const double albedo = (double)(A.albedo ? A.albedo[3u * e + ch] : 1.0f);
      const double lit = ((albedo * E[ch]) * PT_GRID_INV_PI) + add;
      A.color[3u * e + ch] = miss ? (float)((double)A.grid.miss_color[ch] + add) : (valid ? (float)lit : (float)quiet_nan());
    }
  }
}

/* ---- probe updates (rt_hip.h, "probe updates") ---- */

/* the grid index of the round's j-th probe */
__device__ __forceinline__ size_t round_probe(const PtProbeRound &R, uint64_t j) { return (size_t)(R.phase + j * R.stride); }

/* alpha of a probe by its age: the larger of 1 / (age + 1) and 1 - h */
__device__ __forceinline__ double age_alpha(uint32_t age, double h)
{
  const double warm = 1.0 / ((double)age + 1.0), base = 1.0 - h;
  return warm > base ? warm : base;
}

__global__ void __launch_bounds__(PROBE_BLOCK) k_probe_grid_positions_strided(const PtGrid G, const PtProbeRound R, double *__restrict__ positions)
{
  const uint32_t j = blockIdx.x * PROBE_BLOCK + threadIdx.x;
  if (j >= R.m)
    return;
  const uint32_t i = (uint32_t)round_probe(R, j);
  const uint32_t ix = i % G.count[0], r = i / G.count[0], iy = r % G.count[1], iz = r / G.count[1];
  positions[3u * (size_t)j + 0u] = grid_at(G, 0, ix);
  positions[3u * (size_t)j + 1u] = grid_at(G, 1, iy);
  positions[3u * (size_t)j + 2u] = grid_at(G, 2, iz);
}

/* One thread a (probe of the round, basis, channel).  Every thread of a probe works the change rule out again from the probe's three
 * L0 values -- 27 contiguous doubles a probe on both sides, so that a wave's loads stay on whole lines --: a value has one writer.
 * The blend is in place, and the L0 values are read by threads that do not write them: a workgroup holds PROBE_BLEND_PROBES whole
 * probes (243 of its 256 threads), and all of its reads come before its barrier, all of its writes after. */
constexpr uint32_t PROBE_BLEND_PROBES = PROBE_BLOCK / (3u * PT_PROBE_SH);
static_assert(PROBE_BLEND_PROBES >= 1u, "a workgroup of k_probe_coeff_blend holds at least one whole probe");

__global__ void __launch_bounds__(PROBE_BLOCK) k_probe_coeff_blend(const PtProbeCoeffBlend A)
{
  constexpr uint32_t V = 3u * PT_PROBE_SH;
  const uint32_t slot = threadIdx.x / V, r = threadIdx.x - slot * V;
  const uint64_t j_any = (uint64_t)blockIdx.x * PROBE_BLEND_PROBES + slot;
  const bool live = slot < PROBE_BLEND_PROBES && j_any < A.round.m;
  const uint64_t j = live ? j_any : 0u; /* (a thread without a value reads nothing and writes nothing) */
  const size_t i = round_probe(A.round, j);
  const double *__restrict__ const s = A.sum + j * V;
  double *const old = A.coeff + i * V;
  const uint32_t age = live ? A.age[i] : 0u;
  double alpha = age_alpha(age, A.hysteresis);
  const double fresh = live ? (s[r] * A.inv_samples) * A.k : 0.0;
  double out = fresh, change_out = 1.0;
  const bool blends = age != 0u; /* (a probe that starts over does not read its old state) */
  const double old_r = blends ? old[r] : 0.0, o0 = blends ? old[0] : 0.0, o1 = blends ? old[1] : 0.0, o2 = blends ? old[2] : 0.0;
  __syncthreads();
  if (!live)
    return;
  if (blends)
  {
    const double o3[3] = {o0, o1, o2};
    double c = 0.0, m = 0.0;
#pragma unroll
    for (uint32_t ch = 0; ch < 3u; ch++)
    {
      const double f = (s[ch] * A.inv_samples) * A.k, o = o3[ch];
      const double d = fabs(f - o), af = fabs(f), ao = fabs(o), big = af > ao ? af : ao;
      c = d > c ? d : c;
      m = big > m ? big : m;
    }
    change_out = m > 0.0 ? c / m : 0.0;
    if (A.change > 0.0 && c > A.change * m)
    {
      const double quick = 1.0 - A.fast;
      alpha = alpha > quick ? alpha : quick;
    }
    const double keep = 1.0 - alpha;
    out = (old_r * keep) + (fresh * alpha);
  }
  old[r] = out;
  if (A.coeff_f)
    A.coeff_f[i * V + r] = (float)out;
  if (A.change_out && r == 0u)
    A.change_out[i] = change_out;
}

/* One thread a (probe of the round, texel): the moment pair is loaded and stored as 16 bytes.  A texel the round says nothing about
 * (W == 0) is not stored at all unless the probe starts over. */
__global__ void __launch_bounds__(PROBE_BLOCK) k_probe_moment_blend(const PtProbeMomentBlend A)
{
  const uint32_t texels = A.res * A.res;
  const uint64_t t = (uint64_t)blockIdx.x * PROBE_BLOCK + threadIdx.x;
  if (t >= (uint64_t)A.round.m * texels)
    return;
  const uint64_t j = t / texels;
  const uint32_t texel = (uint32_t)(t - j * texels);
  const size_t i = round_probe(A.round, j);
  const double *__restrict__ const s = A.sums + (j * texels + texel) * 3u;
  double2 *const at = reinterpret_cast<double2 *>(A.moments) + (i * texels + texel);
  const uint32_t age = A.age[i];
  const double alpha = age_alpha(age, A.hysteresis);
  const double W = s[0], M1 = s[1], M2 = s[2];
  double2 out;
  if (W != W)
    out.x = out.y = W;
  else if (W > 0.0)
  {
    out.x = M1 / W;
    out.y = M2 / W;
    if (age != 0u)
    {
      const double2 old = *at;
      const double keep = 1.0 - alpha;
      out.x = (old.x * keep) + (out.x * alpha);
      out.y = (old.y * keep) + (out.y * alpha);
    }
  }
  else if (age == 0u)
  {
    out.x = A.d_max;
    out.y = A.d_max * A.d_max;
  }
  else
    return;
  *at = out;
}

__global__ void __launch_bounds__(PROBE_BLOCK) k_probe_age_step(const PtProbeRound R, uint32_t *__restrict__ age,
                                                                 const uint32_t *__restrict__ round_status, uint32_t *__restrict__ status)
{
  const uint32_t j = blockIdx.x * PROBE_BLOCK + threadIdx.x;
  if (j >= R.m)
    return;
  const size_t i = round_probe(R, j);
  const uint32_t a = age[i];
  age[i] = a == 0xFFFFFFFFu ? a : a + 1u;
  if (round_status && status)
    status[i] = round_status[j];
}

uint32_t blocks_for(uint64_t threads) { return (uint32_t)((threads + PROBE_BLOCK - 1u) / PROBE_BLOCK); }

} // namespace

hipError_t probe_launch_grid_positions_strided(const PtGrid &grid, const PtProbeRound &round, double *positions, hipStream_t stream)
{
  hipLaunchKernelGGL(k_probe_grid_positions_strided, dim3(blocks_for(round.m)), dim3(PROBE_BLOCK), 0, stream, grid, round, positions);
  return hipGetLastError();
}

hipError_t probe_launch_coeff_blend(const PtProbeCoeffBlend &args, hipStream_t stream)
{
  const uint32_t blocks = (args.round.m + PROBE_BLEND_PROBES - 1u) / PROBE_BLEND_PROBES;
  hipLaunchKernelGGL(k_probe_coeff_blend, dim3(blocks), dim3(PROBE_BLOCK), 0, stream, args);
  return hipGetLastError();
}

hipError_t probe_launch_moment_blend(const PtProbeMomentBlend &args, hipStream_t stream)
{
  const uint64_t threads = (uint64_t)args.round.m * args.res * args.res;
  hipLaunchKernelGGL(k_probe_moment_blend, dim3(blocks_for(threads)), dim3(PROBE_BLOCK), 0, stream, args);
  return hipGetLastError();
}

hipError_t probe_launch_age_step(const PtProbeRound &round, uint32_t *age, const uint32_t *round_status, uint32_t *status, hipStream_t stream)
{
  hipLaunchKernelGGL(k_probe_age_step, dim3(blocks_for(round.m)), dim3(PROBE_BLOCK), 0, stream, round, age, round_status, status);
  return hipGetLastError();
}

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

hipError_t probe_launch_grid_positions(const PtGrid &grid, double *positions, hipStream_t stream)
{
  const uint64_t n = (uint64_t)grid.count[0] * grid.count[1] * grid.count[2];
  hipLaunchKernelGGL(k_probe_grid_positions, dim3(blocks_for(n)), dim3(PROBE_BLOCK), 0, stream, grid, positions);
  return hipGetLastError();
}

hipError_t probe_launch_shade(const PtProbeShade &args, hipStream_t stream)
{
  hipLaunchKernelGGL(k_probe_shade, dim3(blocks_for(args.m)), dim3(PROBE_BLOCK), 0, stream, args);
  return hipGetLastError();
}

hipError_t probe_launch_depth_fold(const PtProbeDepthFold &args, hipStream_t stream)
{
  const uint64_t threads = args.n_probes * args.vis.res * args.vis.res;
  hipLaunchKernelGGL(k_probe_depth_fold, dim3(blocks_for(threads)), dim3(PROBE_BLOCK), 0, stream, args);
  return hipGetLastError();
}

hipError_t probe_launch_depth_resolve(const double *sum, uint64_t n_texels, double d_max, double *moments, hipStream_t stream)
{
  hipLaunchKernelGGL(k_probe_depth_resolve, dim3(blocks_for(n_texels)), dim3(PROBE_BLOCK), 0, stream, sum, n_texels, d_max, moments);
  return hipGetLastError();
}

hipError_t probe_launch_shade_vis(const PtProbeShadeVis &args, hipStream_t stream)
{
  hipLaunchKernelGGL(k_probe_shade_vis, dim3(blocks_for(args.shade.m)), dim3(PROBE_BLOCK), 0, stream, args);
  return hipGetLastError();
}

hipError_t probe_launch_emission(const uint32_t *object, uint64_t n, const double *emission, uint32_t stride, uint32_t n_objects, float *add,
                                 hipStream_t stream)
{
  hipLaunchKernelGGL(k_probe_emission, dim3(blocks_for(3u * n)), dim3(PROBE_BLOCK), 0, stream, object, 3u * n, emission, stride, n_objects, add);
  return hipGetLastError();
}

hipError_t probe_launch_tonemap(const float *rgb, uint64_t n_values, uint8_t *rgb8, hipStream_t stream)
{
  hipLaunchKernelGGL(k_probe_tonemap, dim3(blocks_for(n_values)), dim3(PROBE_BLOCK), 0, stream, rgb, n_values, rgb8);
  return hipGetLastError();
}

hipError_t probe_launch_pixel_centres(uint32_t width, uint32_t height, double *uv, hipStream_t stream)
{
  const uint64_t n = (uint64_t)width * height;
  hipLaunchKernelGGL(k_probe_pixel_centres, dim3(blocks_for(n)), dim3(PROBE_BLOCK), 0, stream, width, (uint32_t)n, (double)width - 1.0,
                     (double)height - 1.0, uv);
  return hipGetLastError();
}

/* ray_store.h -- how a generator kernel writes its wave's rays: 6 doubles a ray, as rt_hip_trace_rays takes them.  A wave's 64 rays
 * are 192 pieces of 16 bytes: they change lanes (ds_bpermute, no LDS allocated) so that each of the wave's three stores writes 1 KB in
 * a row.  Every lane of the wave must reach the call: a lane beyond the range computes the range's last ray again and stores nothing.
 * Included by lens.hip (k_lens_rays) and probe.hip (k_probe_rays) after pt_math.h.  Device code for gfx950 only. */
#ifndef RAY_STORE_H
#define RAY_STORE_H

namespace
{

/* 16 bytes of a ray as the stores move them: two doubles' bits */
struct Piece
{
  unsigned long long a, b;
};

__device__ __forceinline__ Piece piece_of(double a, double b) { return {(unsigned long long)__double_as_longlong(a), (unsigned long long)__double_as_longlong(b)}; }
/* the piece lane `from` holds, under `keep` (all ones or zero); wave-uniform control flow: every lane takes part */
__device__ __forceinline__ Piece piece_from(Piece v, uint32_t from, unsigned long long keep)
{
  return {__shfl(v.a, (int)from) & keep, __shfl(v.b, (int)from) & keep};
}

/* Lane `lane` holds the ray (origin o, direction d) of index wave_first + lane of the buffer `rays`; the wave's first in_wave (1 .. 64)
 * rays are written.  Ray r of the wave is pieces 3r .. 3r + 2; store j writes pieces [64 j, 64 j + 64), lane l the piece 64 j + l. */
__device__ __forceinline__ void store_wave_rays(double *rays, size_t wave_first, uint32_t lane, uint32_t in_wave, V3 o, V3 d)
{
  const Piece m0 = piece_of(o.x, o.y), m1 = piece_of(o.z, d.x), m2 = piece_of(d.y, d.z);
  Piece *const out = reinterpret_cast<Piece *>(rays) + 3u * wave_first;
#pragma unroll
  for (uint32_t j = 0; j < 3u; j++)
  {
    const uint32_t piece = 64u * j + lane, from = piece / 3u, part = piece - 3u * from;
    /* (masks, not a three-way select: the compiler turns that into an indexed array in scratch) */
    const Piece q0 = piece_from(m0, from, part == 0u ? ~0ull : 0ull), q1 = piece_from(m1, from, part == 1u ? ~0ull : 0ull),
                q2 = piece_from(m2, from, part == 2u ? ~0ull : 0ull);
    const Piece q = {q0.a | q1.a | q2.a, q0.b | q1.b | q2.b};
    if (piece < 3u * in_wave)
      out[piece] = q;
  }
}

} // namespace

#endif /* RAY_STORE_H */

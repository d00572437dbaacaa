/* pt_device.h -- device-side data layout shared by the kernels and the shim.
 *
 * HBM layout of a scene (RtHipScene), built once by rt_hip_scene_create() as one blob:
 *
 *   entry_src  [n_spheres + n_triangles] x 6 f64 : cx, cy, cz, R2, |c|, Rb   (scan order)
 *       sphere  : centre, radius*radius (the product raytracer.c:87 forms per test; forming
 *                 it once is the same double), |centre|, 0
 *       triangle: centre / squared radius / radius of a bounding sphere (filter only)
 *       The first four doubles of the sphere records are what the exact test and the
 *       normal use; they are staged in LDS per workgroup (scenes beyond the 24 KiB staging
 *       budget -- and sphere-only scenes beyond ~85 spheres by preference, pt_prefer_streaming --
 *       read the compact copy geom4 from memory instead).
 *   filt       [ceil(entries/2)] x 6 f32x2 (+ [n_triangles] x 16 f32, see pt_filt_bytes) : cx cy cz r2_hi neg_tol kq, two primitives
 *       per f32x2 -- the packed-fp32 phase-1 filter table (pt_build_filter).  Its thresholds depend
 *       on the camera distance (near_R), so the shim keeps one table set per (scene, near_R),
 *       built once and immutable afterwards; staged in LDS by small scenes, otherwise read with
 *       wave-uniform indices through the constant address space, i.e. by scalar loads
 *       (pt_filter.h, ConstPair: as plain global loads they had been compiled to vector loads).
 *   material   [n_spheres + n_meshes] x 8 f64    : prob, albedo_rr xyz, emission xyz, flags
 *       prob      = MAX(color) (raytracer.c:497)
 *       albedo_rr = color * (1/prob), the albedo after a survived Russian roulette (:500);
 *                   same operands, same two operations as the reference performs per
 *                   bounce, so the same doubles.
 *   color_raw  [n_spheres + n_meshes] x 3 f64    : the colours as given; cast_ray
 *                   (raytracer.c:574) shades with them, trace_path never reads them.
 *   tri_geom   [n_triangles] x 9 f64 : v0, edge1 = v1-v0, edge2 = v2-v0
 *       (raytracer.c:132-133 forms the edges per test; precomputed = same).
 *   tri_normal [n_triangles] x 3 f64 : calculate_surface_normal(v0,v1,v2)
 *       (raytracer.c:42-45), read only for the winning triangle.
 *   tri_tex    [n_triangles] x 6 f64 : st0, st1, st2 (read only for a winning triangle of an
 *       M_CHECKERED mesh).
 *   tri_object [n_triangles] u32     : material slot of the owning mesh; bits 31 / 30 (PT_HULL_PLUS / PT_HULL_MINUS,
 *       set on the device by pt_build_hull_flags): every triangle of the scene lies on the inner side of this
 *       triangle's plane, the stored normal pointing out / in -- a ray that leaves such a HULL FACET on its outer
 *       side cannot meet a triangle again.
 *   bvh_src    [n_bvh_nodes] x 16 f64 : a binary bounding-volume hierarchy over the triangles
 *       (built for every scene that has any; the small-scene kernels scan triangles through
 *       the flat filter and ignore it).  A node holds the boxes of its TWO children
 *       (child 0: min xyz, max xyz; child 1: the same) and their references packed as two u32
 *       in double 12: an inner child is its node index, a leaf child is
 *       PT_BVH_LEAF_FLAG | first << PT_BVH_COUNT_BITS | count and covers bvh_tri[first .. first+count).  Node 0
 *       is the root; the tree is balanced (median splits), depth <= PT_BVH_STACK.
 *   bvh_nodes  [n_bvh_nodes] x 16 u32/f32 : the fp32 copy for one near_R (pt_build_bvh): the six
 *       planes as (child 0, child 1) pairs -- min x, max x, min y, max y, min z, max z -- so one
 *       packed-fp32 instruction serves both children; boxes widened by a bound on the fp32
 *       ray/box arithmetic; then the two references.
 *   bvh_tri    [n_triangles] u32     : triangle indices in leaf order.
 */
#ifndef PT_DEVICE_H
#define PT_DEVICE_H

#include <math.h>
#include <stdint.h>

#define PT_TILE 8
#define PT_TILE_PIXELS 64
#define PT_SLICES 4         /* sample slices per pixel inside one wavefront */
#define PT_BLOCK 256        /* 4 wavefronts: 64 pixels x 4 slices */
#define PT_MAT_STRIDE 8     /* doubles per material record */
#define PT_MAT_EMISSION 4   /* ... of which doubles 4 .. 6 are the emission (x, y, z) */
#define PT_FILT_LDS_MAX 256  /* primitives up to which the filter table is also staged in LDS */
#ifndef PT_BVH_LEAF
#define PT_BVH_LEAF 15        /* max triangles per BVH leaf (< 2^PT_BVH_COUNT_BITS); config 5 at 4K x 256 spp: 2: 435 ms,
                               * 3: 428, 4: 428, 7: 420 (round 1's kernel).  With the pipelined fp32 pre-test at the leaves
                               * (round 2: a leaf visit costs one exposed round trip whatever its size) at 64 / 256 spp:
                               * 2: 88.3 / 326.7 ms, 4: 86.5 / 321.0, 7 (5 per leaf in config 5): 71.9 / 268.2,
                               * 15 with PT_BVH_COUNT_BITS 4 (10 per leaf): 71.4 / 266.8, 31 with 5 bits (20 per leaf): 73.2 / 273.9.
                               * End of round 3 (node visits and pre-tests trimmed, the walk waits for its node fetches more
                               * than it computes): 4: 70.2 / 261.1 ms, 7: 58.5 / 219.3, 15: 58.4 / 217.7, 31: 60.3 / 225.3 -> 15 */
#endif
#define PT_BVH_NODE_WORDS 16  /* 64-byte device node: 6 f32x2 planes (child 0, child 1) + 2 refs + pad */
#define PT_BVH_SRC_DOUBLES 16 /* fp64 source node: 2 x (min xyz, max xyz), refs, pad */
#ifndef PT_BVH_COUNT_BITS
#define PT_BVH_COUNT_BITS 4 /* bits of a leaf reference that hold its triangle count (PT_BVH_LEAF < 2^bits) */
#endif
#define PT_BVH_LEAF_FLAG 0x80000000u
#define PT_BVH_STACK 24       /* per-lane traversal stack (LDS): tree depth limit */
#define PT_GEOM_STRIDE 4     /* LDS doubles per sphere: cx cy cz r2 */
#define PT_FILT_STRIDE 6     /* HBM f32x2 per primitive PAIR: cx cy cz r2_hi neg_tol kq (phase-1 filter; kq = |c|^2 - r2_hi of the sign-test form) */
#define PT_TRI32_STRIDE 16    /* floats per triangle of the fp32 pre-test table: v0 e1 e2 (9), Ea KU KV KT (4), pad (3) */
#define PT_ENTRY_SRC_STRIDE 6 /* HBM doubles per primitive: cx cy cz R2 |c| Rb (bounding data, fp64) */

/* parked-walk kernels (pt_render_tiles_tri_queued*): bytes of ring per wave in the workspace, slots
 * (workgroups) per XCD the pool provides: 32 CUs x at most 5 resident workgroups, with slack */
#define PT_PARK_WIN_BYTES 9216u /* the refraction form's windowed pixel sums of the wave's tile: 64 pixels x 3 channels x 6 words (the LAST bytes of a wave's region) */
#ifndef PT_PARK_WAVE_BYTES
#define PT_PARK_WAVE_BYTES (65536u + 512u + PT_PARK_WIN_BYTES) /* 512 entries of 128 bytes (pt_body_queued.h, PT_PARK_Q: why 512), then the tile's 64 per-pixel RNG keys, then the windows */
#endif
/* slots per XCD of the two pools (this one and the pending-ray pool below): derived per device from the occupancy of the kernels
 * that take slots, with 25 % slack (pt_pool_slots_per_xcd).  The development build (librt_hip_dev.so) takes RT_HIP_POOL_SLOTS=n
 * instead: with n = 1 acquisition FAILS for all but eight workgroups, which is how the failure path is tested. */
#define PT_PARK_XCDS 8u
/* device-side failures a launch can report through PtLaunch.status (rt_hip.h: RT_HIP_FAIL_*) */
#define PT_FAIL_PEND_SLOT 1u
#define PT_FAIL_PARK_SLOT 2u

#define PT_HULL_PLUS 0x80000000u
#define PT_HULL_MINUS 0x40000000u
#define PT_HULL_MAX_TRIS 65536u /* pt_build_hull_flags is quadratic: larger triangle sets go without the flags */
#define PT_ACC_WS_WORDS (PT_TILE_PIXELS * 3 + 3) /* chunked renders: u64 per tile in the workspace: 192 sums + 3 NaN masks */
#define PT_WIN_N 6 /* words of a windowed pixel-channel sum (pt_scene_ctx.h, win_add): the M_REFRACTION forms of the pooled and parked-walk kernels */
#define PT_ACC_WS_WORDS_WIN (PT_TILE_PIXELS * 3 * PT_WIN_N + 3) /* ... whose chunked renders keep 192 x PT_WIN_N words + 3 NaN masks per tile */

#define PT_REFRACT_MAX_DEPTH 32 /* the pending-ray stacks of the two-child kernels hold max_depth + 2 entries (a pool in global memory
                                 * sized by the launch: 20 KB per entry and resident workgroup) */
#define PT_PEND_FIELDS_HOST 10u /* doubles per pending ray: o, d, T, depth (pt_scene_ctx.h: PT_PEND_FIELDS) */
#define PT_PEND_COLUMNS 512u /* stacks per pool slot: the static body uses one per lane (256), the pooled refraction kernel 128 per wave */
#if defined(__HIPCC__)
__host__ __device__
#endif
static inline bool pt_refr_pool_fits(int32_t samples, int32_t max_depth)
{ /* pt_scene_ctx.h, win_add: a window word holds 2^31 pieces (each below 2^32: |sum| < 2^63).  Every event of a path can add one
   * term, i.e. one piece per word, and every refractive hit of a sample starts one more path: a sample is at most a full binary
   * tree of max_depth + 2 levels, 2^(max_depth + 2) - 1 terms.  The rule keeps samples x 2^(max_depth + 1) <= 2^30, so a chunk
   * adds at most 2^31 pieces to a word: exactly the capacity, no margin beyond it (tests/test_gpu_parity.py checks the
   * capacity itself through rt_hip_selftest_math op 8).  (`samples`: of one sample chunk; until round 5 the rule was
   * 2^(max_depth + 2) on a launch's whole sample count.) */
  return max_depth + 1 <= 30 && ((int64_t)samples << (max_depth + 1)) <= ((int64_t)1 << 30);
}
/* the fewest sample chunks with which a launch of `samples` per pixel fits the rule; 0: none does (max_depth > 29) */
#if defined(__HIPCC__)
__host__ __device__
#endif
static inline uint32_t pt_refr_pool_chunks_needed(int32_t samples, int32_t max_depth)
{
  if (max_depth + 1 > 30 || samples < 1)
    return 0u;
  const int64_t per_chunk = ((int64_t)1 << 30) >> (max_depth + 1); /* >= 1 */
  return (uint32_t)(((int64_t)samples + per_chunk - 1) / per_chunk);
}

/* ---- the pixel sums a trace_path launch can use (host side: pt_classify and the launch read the same functions) ----------
 * Fixed point (fixed_term, pt_math.h): every term of a sample is bounded by per_sample = (max_depth + 2) x max(BACKGROUND,
 * max |emission|) x 1.01 (throughput <= 1 without M_REFRACTION; at most max_depth + 2 events).  The scale is 2^s, the largest
 * power of two with samples x per_sample x 2^s < 2^62 (the sum) and per_sample x 2^s < 2^51 (a term read off an fp64
 * mantissa).  -> s; INT32_MIN when the bound is not a finite positive number. */
static inline int pt_acc_scale_exp(double max_emission, int32_t samples, int32_t max_depth)
{
  const double per_sample = ((double)max_depth + 2.0) * fmax(10.0 / 255.0, max_emission) * 1.01;
  const double bound = per_sample * (double)samples;
  if (!(bound > 0) || !(bound < 1e300))
    return INT32_MIN;
  int e = 0, e1 = 0;
  (void)frexp(4611686018427387904.0 / bound, &e);    /* 2^62 / bound = m * 2^e, m in [0.5, 1) */
  (void)frexp(2251799813685248.0 / per_sample, &e1); /* 2^51 / per_sample */
  return (e1 < e ? e1 : e) - 1;
}
/* A term is rounded to a multiple of 2^-s, so a pixel mean is off by up to (max_depth + 2) x 2^-s / 2.  The brightest emitter
 * sets s whether or not a ray can reach it: at 1e15 a pixel of BACKGROUND rounds to 0.  The fixed-point sums are kept while that
 * error is <= 2^-30 (float32's half ulp at 1/64; the baseline launches sit at 2^-31.8, config 4 at 1024 spp and depth 16, and
 * 2^-30.8, config 5 at 4096 spp); beyond it the launch takes the windowed or fp64 sums of the M_REFRACTION forms, exact
 * above 2^-64 (pt_classify). */
static inline bool pt_fixed_sums_fit(double max_emission, int32_t samples, int32_t max_depth)
{
  const int s = pt_acc_scale_exp(max_emission, samples, max_depth);
  return s != INT32_MIN && ldexp((double)max_depth + 2.0, -s - 1) <= ldexp(1.0, -30);
}
/* win_add refuses a term of 2^128 or more (it flags the pixel): scenes whose bound reaches that keep fp64 sums (the static kernels) */
static inline bool pt_window_terms_fit(double max_emission, int32_t max_depth)
{
  return ((double)max_depth + 2.0) * fmax(10.0 / 255.0, max_emission) * 1.01 < 3.402823669209385e38; /* 2^128 */
}

#define PT_FLAG_DIFFUSE 2u
#define PT_FLAG_MIRROR 4u
#define PT_FLAG_REFRACT 8u
#define PT_FLAG_CHECKER 16u

struct PtSceneView
{
  const double *entry_src; /* n_spheres + n_triangles bounding records, scan order */
  const double *geom4;     /* n_spheres x PT_GEOM_STRIDE: cx cy cz r2, what the exact test reads when the
                            * scene is too large to stage in LDS */
  float *filt;             /* packed-fp32 filter table for the launch's near_R (pt_build_filter; the shim keeps one
                            * immutable table set per (scene, near_R)) */
  const double *material;
  const double *color_raw;
  const double *tri_geom;
  const double *tri_normal;
  const double *tri_tex;
  const uint32_t *tri_object;
  const double *bvh_src;
  float *bvh_nodes;
  const uint32_t *bvh_tri;
  const double *tri_geom_leaf; /* n_triangles x 9: tri_geom in LEAF order (entry k belongs to triangle bvh_tri[k]), so a leaf's
                                * triangles are contiguous and their loads do not wait for the index load */
  uint32_t n_spheres, n_meshes, n_triangles, any_checker;
  /* the triangles' bounding sphere shows a ray no more than their bounding box does on average (pi R^2 against
   * (ab + bc + ca) / 2): the parked-walk kernel's probe then tests the sphere alone (pt_render_tiles_tri_queued_sph) */
  uint32_t mesh_round;
  uint32_t any_refract, n_bvh_nodes; /* n_bvh_nodes == 0: the scene has no triangles */
  uint32_t wide_range;               /* a centre or radius beyond 1e17: fp32 sums could overflow */
  uint32_t any_mirror_glass;         /* a material with M_REFLECTION and M_REFRACTION: cast_ray traces two children per hit */
  uint32_t bvh_depth;                /* inner nodes on the longest root-to-leaf path: the traversal stack a lane needs */
};
/* Small scenes keep the filter table in LDS and (sphere-only ones) use the sign-test form of
 * the filter, whose NaN-free argument needs every |c|, r <= 1e17; everything else streams the
 * table through scalar loads and keeps the NaN-safe compares. */
#if defined(__HIPCC__)
__host__ __device__
#endif
#ifndef PT_GEOM_LDS_BYTES
#define PT_GEOM_LDS_BYTES (24u * 1024u) /* the LDS staging budget of sphere geometry + materials */
#endif
static inline bool pt_geom_in_lds(const PtSceneView &sc)
{ /* sphere geometry + materials within the staging budget */
  return (PT_GEOM_STRIDE * (uint64_t)sc.n_spheres + PT_MAT_STRIDE * ((uint64_t)sc.n_spheres + sc.n_meshes)) * 8u <= PT_GEOM_LDS_BYTES;
}
#if defined(__HIPCC__)
__host__ __device__
#endif
/* Sphere-only scenes of more than ~85 spheres are better off NOT staged although they would fit: a workgroup's life is
 * short (64 pixels x spp), staging copies 120 bytes per sphere into LDS for each of the frame's tens of thousands of
 * workgroups, and the staged bytes cost resident workgroups (256 spheres: 3 per CU instead of 5).  The pooled body that reads
 * geometry and materials from memory and the filter table through scalar loads (pt_render_tiles_pool_mem_s) measured, per
 * sphere test at 1920x1080 x 64 spp in rooms packed as main.c:65-138 would (profiles/r04_staging_sweep.txt): 10 spheres
 * 1.88 ps against 1.84 staged, 38: 0.660 / 0.634, 64: 0.455 / 0.463, 128: 0.327 / 0.375, 192: 0.284 / 0.327, 256: 0.267 / 0.389.
 * (The pooled sphere kernels only: scenes with triangles, M_REFRACTION or cast_ray keep the staging budget.) */
#ifndef PT_STREAM_ABOVE_BYTES
#define PT_STREAM_ABOVE_BYTES (8u * 1024u)
#endif
#if defined(__HIPCC__)
__host__ __device__
#endif
static inline bool pt_stream_sized(const PtSceneView &sc)
{ /* a sphere scene large enough to be better off streamed */
  return sc.n_triangles == 0u && !sc.wide_range &&
         (PT_GEOM_STRIDE * (uint64_t)sc.n_spheres + PT_MAT_STRIDE * ((uint64_t)sc.n_spheres + sc.n_meshes)) * 8u > PT_STREAM_ABOVE_BYTES;
}
#if defined(__HIPCC__)
__host__ __device__
#endif
static inline bool pt_prefer_streaming(const PtSceneView &sc) { return pt_stream_sized(sc) && !sc.any_refract; } /* (refractive ones: pt_render_tiles_refr_pool_mem, pt_pick_kernel) */
#if defined(__HIPCC__)
__host__ __device__
#endif
static inline bool pt_filter_in_lds(const PtSceneView &sc)
{
  return (uint64_t)sc.n_spheres + sc.n_triangles <= PT_FILT_LDS_MAX && !sc.wide_range && pt_geom_in_lds(sc);
}

/* Sign-test form of the phase-1 filter (small sphere scenes; pt_build_filter writes the table, the kernels' BigPrune
 * and the host's big_prune_for reason about it): how far a sphere's squared radius is widened in its table entry
 * kq = |c|^2 - r2_hi', with e = 2^-24, A = |c| + near_R and g = | |c|^2 - r^2 |.  ONE definition for the device code that
 * builds the table and the host code that bounds hit-distance estimates by it (round-3 advisor finding: the two used to
 * be maintained by hand in separate files):
 *   pt_sign_widen_r2    what is added to r^2 before the subtraction from |c|^2 (the fp32 arithmetic's error bound,
 *                       derivation at pt_build_filter);
 *   pt_sign_widen_kq    what is taken off kq afterwards, for the chain's own roundings of kq;
 *   pt_sign_widen_total their sum: r2_hi' - r^2 as the table has it, before kq's final rounding DOWN to fp32 (one more
 *                       2 e |kq|: callers that need an upper bound on the widening multiply by 1.001). */
#define PT_E32 5.9604644775390625e-08 /* 2^-24 */
#if defined(__HIPCC__)
__host__ __device__
#endif
static inline double pt_sign_widen_r2(double A, double g) { return (40.0 * PT_E32 * A * A + 8.0 * PT_E32 * g) * (1.0 + 8.0 * PT_E32); }
#if defined(__HIPCC__)
__host__ __device__
#endif
static inline double pt_sign_widen_kq(double g) { return 4.0 * PT_E32 * g; }
#if defined(__HIPCC__)
__host__ __device__
#endif
static inline double pt_sign_widen_total(double A, double g) { return pt_sign_widen_r2(A, g) + pt_sign_widen_kq(g); }

/* Phase 1 of the small spheres on the fp16 matrix pipe (pt_filter.h, filter_mfma16; -DPT_MFMA16=1 builds only): a sphere's
 * row of the A operand of v_mfma_f32_32x32x16_f16, 16 halves
 *     k:  0    1    2    3    4    5    6    7  |  8    9  10  11   12   13   14 15
 *         cxh  cyh  czh  cxh  cyh  czh  cxl  cyl | czl   1   1   1   kqh  kql   0  0
 * against the ray's  xh yh zh xl yl zl xh yh | zh p1 p2 p3 s s 0 0  with (x, p, s) = (d, -o'.d in three parts, 0) for tca' and
 * (-2 o', |o'|^2 in three parts, 1) for ll: every product but lo x lo, accumulated in fp32.  c = hi + lo is the fp64 centre
 * rounded to 22 bits (hi = RN16(c), lo = RN16(c - hi)); kq = kqh + kql EXACTLY, and at most |c|^2 - (r^2 + W16).
 *   The bound behind W16, derived as the one above pt_build_filter (pt_kernel.hip): u = 2^-11, e = 2^-24, A = |c| + near_R + tol (tol = the launch's
 *   filt_shift, the pull-back of the ray's origin: pt_mfma16_row takes it and adds it),
 *   |d| <= 1.0001, the ray's values split by the device with |x - xh - xl| <= 4 u^2 |x| (round to nearest or towards zero) and
 *   |xl| <= 2 u |x|, halves below 2^-14 quantised to 2^-24 (phi = 2^-24 covers a product's two such floors), and the matrix
 *   pipe's sum of K = 16 exact products taken to lose at most one fp32 ulp of the sum of magnitudes per addition,
 *   16 x 2^-23 = 2^-19 in all, whatever the order:
 *     a product:  |ch xh + ch xl + cl xh - c x| <= (u^2 + 4 u^2 + e + 2.01 u^2) |c x| + phi (|c| + |x|) <= 2^-19 |c x| + phi (|c| + |x|);
 *     tca16:  |tca16 - tca'| <= 2^-19 1.0001 |c| + 2^-19 1.02 A + 5.1 e A (o'.d, as for the fp32 form) + 2^-29 A + floors
 *             <= ET = 3 x 2^-19 A + 2^-20;
 *     ll16:   |ll16 - (|c - o'|^2 - r2_hi16)| <= 10 e A^2 + 5 e |kq| (the fp32 values the two forms share) + 2^-19 A^2 / 2 (products,
 *             2 |c||o'| <= A^2 / 2) + 2^-29 A^2 + 2^-19 (|kq| + A^2) + 6 phi A  <= EL = 1.82 x 2^-19 A^2 + 1.16 x 2^-19 |kq| + 6 phi A;
 *     q''16 = fma(tca16, |tca16|, -ll16):  |tca'| <= 1.0001 A, so
 *             |q''16 - (r2_hi16 - d2)| <= ET (2.0002 A + ET) + EL + 2 e (A^2 + |kq|) <= E16 = 8 x 2^-19 A^2 + 1.5 x 2^-19 |kq| + 2^-18 A.
 *   A lane whose tca16 comes out negative although tca' > 0 has tca' <= ET and sees -tca16^2 - ll16 >= W16 - 2 ET^2 - EL: inside
 *   the same bound, so the fp32 form's pull-back of the origin needs no widening.  W16 = 2^-16 A^2 + 2^-18 g + 2^-17 A with
 *   g = | |c|^2 - r^2 | (|kq| <= g + W16): about six times the fp32 form's 40 e A^2, against radii of order 1.
 * A sphere FITS the form (return 1) when everything is finite, its radius is below the wall threshold, |c_i| <= 4096 and
 * |kq| <= 60000 (fp16's range), and near_R <= PT_MFMA16_NEAR_R_MAX so that |o'|^2 < 65504 for every ray that is filtered at all. */
#define PT_MFMA16_NEAR_R_MAX 250.0
#define PT_MFMA16_ROWS 32u
#define PT_WALL_RADIUS 1000.0
#if defined(__HIPCC__)
__host__ __device__
#endif
static inline uint16_t pt_f16_rn(double x) /* round to nearest even; |x| < 65520 and finite */
{
  const uint16_t s = x < 0.0 ? 0x8000u : 0u;
  const double a = fabs(x);
  if (a == 0.0)
    return s;
  int ex;
  (void)frexp(a, &ex); /* a = m 2^ex, m in [0.5, 1) */
  const int q = ((ex - 1 < -14) ? -14 : ex - 1) - 10;
  const double v = ldexp(rint(ldexp(a, -q)), q);
  if (v == 0.0)
    return s;
  (void)frexp(v, &ex);
  const int E = ex - 1;
  if (E < -14)
    return (uint16_t)(s | (uint16_t)ldexp(v, 24));
  return (uint16_t)(s | (uint16_t)(((E + 15) << 10) + ((int)ldexp(v, 10 - E) - 1024)));
}
#if defined(__HIPCC__)
__host__ __device__
#endif
static inline double pt_f16_value(uint16_t h)
{
  const int E = (h >> 10) & 31, m = h & 1023;
  const double v = E == 0 ? ldexp((double)m, -24) : ldexp((double)(m + 1024), E - 25);
  return (h & 0x8000u) ? -v : v;
}
#if defined(__HIPCC__)
__host__ __device__
#endif
static inline double pt_mfma16_widen(double A, double g)
{
  return (A * A / 65536.0 + g / 262144.0 + A / 131072.0) * (1.0 + 1e-6);
}
/* src = cx cy cz r^2 |c| . (an entry_src record); tol = the launch's filt_shift, by which the ray's origin is pulled back (part of A);
 * row[16] as laid out above */
#if defined(__HIPCC__)
__host__ __device__
#endif
static inline int pt_mfma16_row(const double *src, double near_R, double tol, uint16_t row[16])
{
  for (int k = 0; k < 16; k++)
    row[k] = 0;
  const double cn = src[4], r2 = src[3];
  if (!(near_R <= PT_MFMA16_NEAR_R_MAX) || !(tol >= 0.0) || !(tol <= 1.0) || !(cn <= 8192.0) || !(r2 >= 0.0) || !(r2 < PT_WALL_RADIUS * PT_WALL_RADIUS))
    return 0;
  uint16_t hi[3], lo[3];
  for (int a = 0; a < 3; a++)
  {
    if (!(fabs(src[a]) <= 4096.0))
      return 0;
    hi[a] = pt_f16_rn(src[a]);
    lo[a] = pt_f16_rn(src[a] - pt_f16_value(hi[a]));
  }
  const double A = (cn + near_R + tol) * (1.0 + 1e-6), cc = cn * cn, g = fabs(cc - r2);
  double kq = cc - (r2 + pt_mfma16_widen(A, g));
  kq -= fabs(kq) / 2097152.0 + 1.0 / 8388608.0; /* the split's own residual (<= 2^-22 |kq| + 2^-25), taken off beforehand */
  if (!(fabs(kq) <= 60000.0))
    return 0;
  const uint16_t kh = pt_f16_rn(kq), kl = pt_f16_rn(kq - pt_f16_value(kh));
  const uint16_t one = 0x3C00u;
  row[0] = row[3] = hi[0];
  row[1] = row[4] = hi[1];
  row[2] = row[5] = hi[2];
  row[6] = lo[0];
  row[7] = lo[1];
  row[8] = lo[2];
  row[9] = row[10] = row[11] = one;
  row[12] = kh;
  row[13] = kl;
  return 1;
}

/* The filter buffer of a small scene (pt_filter_in_lds) holds two tables: the pair table of
 * phase 1 (PT_FILT_STRIDE f32x2 per primitive pair, + the look-ahead pair), then, 16-byte aligned,
 * the fp32 triangle table of the per-lane pre-test (PT_TRI32_STRIDE floats per triangle). */
#if defined(__HIPCC__)
__host__ __device__
#endif
static inline uint32_t pt_filt_pair_slots(uint32_t n_entries)
{ /* f32x2 slots of the pair table, rounded up to a 16-byte boundary */
  return (PT_FILT_STRIDE * ((n_entries + 1u) / 2u + 1u) + 1u) & ~1u;
}
#if defined(__HIPCC__)
__host__ __device__
#endif
static inline size_t pt_filt_bytes(uint32_t n_spheres, uint32_t n_triangles)
{
  return (size_t)pt_filt_pair_slots(n_spheres + n_triangles) * 8u + (size_t)n_triangles * PT_TRI32_STRIDE * 4u;
}

struct PtCamera
{
  double pos[3], horizontal[3], vertical[3], llc[3];
};

struct PtLaunch
{
  PtSceneView scene;
  PtCamera cam;
  int32_t width, height, samples, max_depth;
  uint64_t seed;
  double near_R;  /* the phase-1 filter's assumption |o| <= near_R (rays beyond it skip the filter) */
  /* wave-uniform values formed on the host so they arrive in SGPRs (formed on the device
   * they would occupy -- and spill -- vector registers): near_R^2, width-1, height-1 as the
   * reference forms them, (double)options->width - 1.0 (raytracer.c:203-204) */
  double near_R2, w_minus_1, h_minus_1;
  double filt_shift; /* 12 e (max |c| + near_R): how far behind the origin the sign-test filter starts its ray */
  double hull_margin; /* a ray leaves a hull facet for good if (outward normal) . d exceeds this (rt_hip_shim.hip) */
  uint32_t diag_flags; /* PT_DIAG builds: bit 0 = walk the rays the probe's bounding sphere rejects, to check them; bit 1 = the counters have 64 words (retry-stack counts, slots 44..48).  PT_PHASE builds: bit 2 = the counters hold 80 + 2 x workgroups words and every workgroup of the pooled kernels notes when it began and ended (tools/grid_tail.py) */
  float mesh_bound[5]; /* bvh_probe: the triangles' bounding sphere for this near_R: cx cy cz r2_hi neg_tol (pt_intersect.h, MeshBound) */
  /* two constants passed in so that they live in SGPRs (as literals the compiler parks each in a
   * VGPR pair for the whole loop, and spilled them): BACKGROUND's component 10/255
   * (raytracer.h:46) and DBL_MAX, the initial min_t of intersect() (raytracer.c:396) */
  double background, t_start;
  double inv_w_minus_1, inv_h_minus_1; /* RN(1/(W-1)), RN(1/(H-1)) for div_small_int */
  double acc_scale, acc_inv_scale; /* power-of-two fixed-point scale of the pixel sums */
  uint32_t tile_first, tile_stride, tile_count, tiles_x;
  uint32_t sample_chunks; /* workgroups per tile: each renders 1/sample_chunks of the samples */
  uint32_t acc_windows;   /* sample_chunks > 1: acc_ws holds WINDOWED sums (tile_count x 192 x PT_WIN_N words, then the NaN masks): the M_REFRACTION forms */
  uint32_t integrator;    /* 0 trace_path (raytracer.c:482-554), 1 cast_ray (:556-641) */
  /* accumulation mode (rt_hip_accum_*, rt_hip_shim.hip): a PASS renders the absolute samples [sample_first, sample_first + samples)
   * of every pixel, and with acc_keep set it adds them to the frame's sums and finishes no pixel -- the CHUNKS members into acc_ws
   * (even with one chunk), the static body into slice_ws.  Both zero: a one-shot launch, as before */
  uint32_t sample_first;
  uint32_t acc_keep;
  double *slice_ws; /* static body, acc_keep: tile_count x 3 x PT_BLOCK fp64 slice sums (lane l of tile k, channel c at (3 k + c) x 256 + l), unreduced */
  /* sign-test kernels: the scene's leading pairs of wall-sized spheres (radius >= 1000) are pruned among themselves before
   * the exact tests (pt_filter.h, BigPrune): how many pairs (0: off), the distance margin, the least distance and per sphere the least q32 of a wall that may prune */
  uint32_t big_pairs;
  float big_delta, big_tmin;
  float big_qmin[8];
  /* parked-walk kernels: workspace of PT_PARK_XCDS x park_slots_per_xcd slots x 4 waves x PT_PARK_WAVE_BYTES and
   * one in-use flag per slot (zero between launches).  nullptr (the allocation failed): pt_launch_render takes the
   * lane-waiting _tri_big kernels instead, which need no workspace -- the parked-walk kernels never run without one */
  char *park_ws;
  uint32_t *park_flags;
  uint32_t park_slots_per_xcd;
  /* kernels with two-child materials (M_REFRACTION under trace_path; M_REFLECTION | M_REFRACTION under cast_ray): the pool of
   * pending-ray stacks (pt_scene_ctx.h, PendStack): PT_PARK_XCDS x pend_slots_per_xcd slots of pend_slot_doubles doubles
   * (= pend_entries x 10 fields x PT_BLOCK lanes) and one in-use flag per slot */
  double *pend_ws;
  uint32_t *pend_flags;
  uint32_t pend_slots_per_xcd, pend_entries;
  uint64_t pend_slot_doubles; /* = pend_entries x 10 fields x PT_PEND_COLUMNS */
  /* the device's status word (rt_hip_launch_status): a workgroup that cannot get a pool slot ORs PT_FAIL_* into it, renders
   * nothing and leaves its tile NaN -- the caller gets an error code, not a plausible image */
  uint32_t *status;
  unsigned long long *acc_ws;        /* sample_chunks > 1: tile_count x 192 fixed-point sums, then tile_count x 3 NaN masks */
  float *tiles_rgb;
  uint8_t *tiles_rgb8;
  unsigned long long *stats;
  /* adaptive sampling (rt_hip_accum_freeze): a pass that renders a SET of the frame's slots.  With a list the launch's work units run
   * over slot_count entries instead of tile_count and entry j renders slot slot_list[j] (ascending, each < tile_count); the tile, the
   * pixel keys and every workspace address follow from the slot as before, the NaN masks stay behind tile_count records.  Null / 0 in
   * every launch without frozen tiles; a list needs acc_keep (pt_launch_render) */
  const uint32_t *slot_list;
  uint32_t slot_count;
  /* the mixed grid (the MIXED members, one launch): slots below n_whole run as ONE workgroup each and finish their pixels in the
   * kernel, whatever sample_chunks says; the slots from n_whole on run as sample_chunks workgroups each, dispatched after every whole
   * one, and acc_ws holds records for THOSE slots alone (record slot - n_whole; the NaN masks behind tile_count - n_whole records),
   * which pt_resolve_tiles finishes.  0 in every other launch: the uniform forms, as before.  Needs sample_chunks > 1 and neither
   * acc_keep nor a slot list (pt_launch_render) */
  uint32_t n_whole;
};

/* The compact tile-major outputs of an AOV launch (rt_hip.h, RtHipAov; render_aov in pt_kernel.hip): tile slot k owns albedo / normal
 * [k*192, +192) and depth / object / hits [k*64, +64).  Any pointer may be null (not all: the launcher refuses that). */
struct PtAovOut
{
  float *albedo, *normal, *depth;
  uint32_t *object, *hits;
};

/* One ray query (rt_hip.h, rt_hip_query_rays; query_rays in pt_kernel.hip): n rays in, structure-of-arrays answers out.  rays:
 * n x 6 doubles (origin, direction; 16-byte aligned: a ray is three 16-byte loads) or, with camera_uv, n x 2 doubles (u, v) for the
 * launch's camera.  t_max: n doubles or null (DBL_MAX for every ray).  Any output may be null (not all: the shim refuses that). */
struct PtQuery
{
  const double *rays;
  const double *t_max;
  uint64_t n; /* < 2^32 */
  uint32_t camera_uv, normalize;
  uint32_t *status;
  double *t;
  uint32_t *object, *prim;
  double *point, *normal, *bary, *ray; /* 3, 3, 2, 6 doubles per ray */
};

/* One radiance query (rt_hip.h, rt_hip_trace_rays; trace_sliced<RayFront> in pt_kernel.hip): n rays in as for PtQuery, per ray the mean of
 * PtLaunch.samples trace_path samples out.  Sample s of ray i runs on the stream (PtLaunch.seed, index_first + i, s) after two
 * discarded draws; PtLaunch.max_depth is the reference's MAX_DEPTH.  samples: 3 doubles per (ray, sample), [i * S + s].  paths /
 * casts: per ray, summed over its samples.  Any output may be null (not all: the shim refuses that). */
struct PtTrace
{
  const double *rays;
  uint64_t n; /* < 2^32, index_first + n <= 2^32 */
  uint32_t camera_uv, normalize;
  uint32_t index_first;
  uint32_t *status;
  double *radiance, *samples;
  unsigned long long *paths, *casts;
  double *ray; /* 6 doubles per ray */
};

/* One pixel refinement (rt_hip.h, rt_hip_trace_pixels; trace_sliced<PixelFront> in pt_kernel.hip): n pixel indices in, per entry the mean of
 * PtLaunch.samples samples of the RENDER's own: sample k of entry i is sample sample_first + k of pixel pixels[i] of the launch's
 * width x height frame (start_sample on the stream (PtLaunch.seed, pixel, sample_first + k)).  n_pixels = width * height: an index
 * at or beyond it is invalid.  samples: 3 doubles per (entry, sample), [i * S + k].  Any output may be null (not all). */
struct PtPixels
{
  const uint32_t *pixels;
  uint64_t n; /* < 2^32 */
  uint32_t n_pixels, sample_first;
  uint32_t *status;
  double *radiance, *samples;
  unsigned long long *paths, *casts;
};

/* The ordered compaction of a per-pixel map (rt_hip.h, rt_hip_select_pixels; pt_select_* in image_ops.hip): pixel p of `values` is
 * selected iff (lo <= v && v <= hi) != invert.  A workgroup of pt_select_count / pt_select_scatter covers PT_SELECT_BLOCK pixels, a
 * workgroup of pt_select_scan PT_SELECT_SCAN counts. */
#define PT_SELECT_BLOCK 256u
#define PT_SELECT_SCAN 1024u
struct PtSelect
{
  const float *values;
  uint64_t n; /* pixels, < 2^32 */
  double lo, hi;
  uint32_t invert;
};

/* One blend of traced pixels into a frame (rt_hip.h, rt_hip_blend_pixels; pt_blend_pixels in image_ops.hip) */
struct PtBlend
{
  const uint32_t *pixels, *status;
  const double *radiance;
  uint64_t n; /* entries, < 2^32 */
  uint32_t n_pixels;
  double new_weight, prior_scale;
  const float *prior; /* may be null: 1.0 */
  float *rgb;
  uint8_t *rgb8; /* may be null */
  float *weight; /* may be null; may be `prior` itself */
};

/* One launch of the denoiser (rt_hip.h, rt_hip_denoise; pt_denoise_* in image_ops.hip).  The workspace holds, per pixel of the
 * row-major w x h image: two ping-pong float4 colour buffers e[0], e[1] (the filtered signal, .w = 1 valid / 0 invalid), the
 * guidance float4 (normal, depth) and uint2 (hits, object) the prepare pass packs so that a tap is three loads. */
struct PtDenoise
{
  const float *rgb, *albedo, *normal, *depth; /* inputs: albedo only with DEMODULATE */
  const uint32_t *hits, *object;              /* object only with OBJECT_EDGES */
  float *e[2], *guide;                        /* workspace: 4 floats per pixel each */
  uint32_t *hit_obj;                          /* workspace: 2 words per pixel */
  float *out_rgb;                             /* each may be null, not both */
  uint8_t *out_rgb8;
  int32_t width, height;
  uint32_t demodulate, object_edges, k; /* rt_hip.h: RT_HIP_DENOISE_DEMODULATE, _OBJECT_EDGES (0 / 1), normal_power_log2 */
  double sigma_z;
};

/* One temporal reprojection (rt_hip.h, rt_hip_reproject; pt_reproject in image_ops.hip): row-major w x h images of the frame
 * (colour, normal, depth, hits, object) and of the history (the same and its length; all null together: the first frame), the two
 * cameras, and the outputs -- out_rgb and out_len always, the bytes and the motion (2 floats per pixel) where wanted. */
struct PtReproject
{
  const float *rgb, *normal, *depth;
  const uint32_t *hits, *object;
  const float *hist_rgb, *hist_len, *hist_normal, *hist_depth; /* hist_rgb null: no history */
  const uint32_t *hist_hits, *hist_object;
  float *out_rgb, *out_len;
  uint8_t *out_rgb8; /* may be null */
  float *out_motion; /* may be null */
  int32_t width, height;
  PtCamera cam, hist_cam;
  double max_history, depth_tol, normal_min;
};

/* The previous points of n query hits (rt_hip.h, rt_hip_prev_points; pt_prev_points in image_ops.hip): the hits' status, prim,
 * bary (2 doubles) and point (3 doubles), the previous positions (9 doubles per triangle; may be null with n_triangles 0) and the
 * output, 3 doubles per entry (it may be `point`). */
struct PtPrevPoints
{
  const uint32_t *status, *prim;
  const double *bary, *point, *positions;
  double *out;
  uint64_t n, n_triangles;
};

/* The same with moved spheres (rt_hip.h, rt_hip_prev_points_moved; pt_prev_points_moved in image_ops.hip): the hits' object as
 * well, and the previous and current spheres, 4 doubles each (cx cy cz radius; may be null with n_spheres 0).  spheres_static:
 * the call gave no previous spheres and n_spheres 0 -- a sphere hit copies its point, as pt_prev_points does. */
struct PtPrevPointsMoved
{
  const uint32_t *status, *prim, *object;
  const double *bary, *point, *positions, *spheres_prev, *spheres_cur;
  double *out;
  uint64_t n, n_triangles, n_spheres;
  uint32_t spheres_static;
};

/* One guided upsampling (rt_hip.h, rt_hip_upsample; pt_upsample in image_ops.hip): the low frame's row-major wl x hl images
 * (colour, normal, depth, hits; albedo with demodulate, object with object_edges), the guides of the w x h frame (the same fields
 * without a colour), and the outputs -- out_rgb always, the bytes and the confidence where wanted. */
struct PtUpsample
{
  const float *low_rgb, *low_albedo, *low_normal, *low_depth;
  const uint32_t *low_hits, *low_object;
  const float *albedo, *normal, *depth; /* albedo: read with demodulate only */
  const uint32_t *hits, *object;        /* object: read with object_edges only */
  float *out_rgb;
  uint8_t *out_rgb8; /* may be null */
  float *out_conf;   /* may be null */
  int32_t low_width, low_height, width, height;
  uint32_t demodulate, object_edges, normal_power_log2;
  double sigma_depth;
};

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
/* host-side launchers, defined next to the kernels in pt_kernel.hip (and, under their own heading below, in image_ops.hip) */
size_t pt_render_lds_bytes(const PtSceneView &scene);
/* the chunks a trace_path launch of a scene with M_REFRACTION takes at least when it has a chunk workspace (pt_plan_launch;
 * rt_hip_suggest_chunks_depth suggests as many): pt_refr_pool_chunks_needed where that is a usable chunk count -- at most one
 * chunk per sample, tile_count x chunks within the grid limit -- else 1 (max_depth > 29: the static kernels render it) */
static inline uint32_t pt_refr_chunk_floor(const PtSceneView &scene, int32_t samples, int32_t max_depth, uint32_t tile_count)
{
  if (!scene.any_refract)
    return 1u;
  const uint64_t need = pt_refr_pool_chunks_needed(samples, max_depth);
  return (need >= 1u && need <= (uint64_t)samples && need * tile_count <= 0x7FFFFFFFull) ? (uint32_t)need : 1u;
}
/* The launch plan (pt_kernel.hip: pt_plan_launch): which member of the family runs a launch, with how many sample chunks, and
 * which pools it needs -- the one place these are decided.  What the launch asks ... */
struct PtPlanAsk
{
  uint32_t integrator;        /* 0 trace_path, 1 cast_ray */
  int32_t samples, max_depth; /* samples per pixel of the whole launch */
  double max_emission;        /* max |emission component| over all materials (pt_acc_scale_exp) */
  uint32_t sample_chunks;     /* as requested by the caller */
  bool have_chunk_ws;         /* the caller gave a chunk workspace */
  uint32_t tile_count;
  bool have_park_ws;          /* the parked-walk kernels' ring workspace exists on the device */
  bool wide_pend_ok;          /* the pending-ray pool can be had at 4 x 512 stacks per slot */
};
/* ... and what it gets */
struct PtPlan
{
  int kernel;                          /* index into the family */
  uint32_t sample_chunks;              /* what the kernel runs */
  bool mixed;                          /* the kernel takes a mixed grid (PtLaunch.n_whole > 0) */
  bool windowed;                       /* pixel sums are windowed (win_add): the chunk workspace has PT_ACC_WS_WORDS_WIN words per tile */
  bool queued;                         /* parked walks: a tile per wave */
  uint32_t pend_entries, pend_columns; /* the pending-ray pool it needs (pend_pool_for); 0 entries: none */
};
PtPlan pt_plan_launch(const PtSceneView &scene, const PtPlanAsk &ask);
hipError_t pt_launch_render(const PtLaunch &launch, hipStream_t stream, int which);
/* accumulation (rt_hip_accum_*): whether member `which` keeps its sums in acc_ws (CHUNKS) rather than as slice sums (the static
 * body), and the resolve of the sums its passes left: pt_resolve_tiles or pt_resolve_slices over launch.samples samples
 * (tile_samples: null, or a count per slot that replaces it where nonzero) */
bool pt_kernel_takes_chunks(int which);
/* workgroups of member `which` the current device holds at once for a launch of `scene` (CUs x workgroups a CU takes with the
 * launch's dynamic LDS); 0: not known */
uint32_t pt_resident_workgroups(int which, const PtSceneView &scene);
hipError_t pt_launch_resolve(const PtLaunch &launch, const uint32_t *tile_samples, hipStream_t stream, int which);
/* adaptive sampling: the per-tile error estimate of two resolves (pt_tile_error), and the freeze -- the keep mask from the errors
 * (error == nullptr: `keep` holds the caller's mask), then the live slots frozen or compacted into slot_list (pt_tile_compact).
 * tile_samples: per slot, 0 = live, else the count it froze at (device, tile_count words) */
hipError_t pt_launch_tile_error(const float *cur, const float *prev, int width, int height, uint32_t tile_first, uint32_t tile_stride,
                                uint32_t tile_count, float *error, hipStream_t stream);
hipError_t pt_launch_tile_freeze(const float *error, double threshold, int dilate, uint8_t *keep, uint32_t *tile_samples, int width,
                                 int height, uint32_t tile_first, uint32_t tile_stride, uint32_t tile_count, uint32_t done,
                                 uint32_t *slot_list, uint32_t *live_count, hipStream_t stream);
/* entries per pending-ray stack a launch needs: max_depth + 2 where a material has two children (M_REFRACTION under trace_path,
 * M_REFLECTION | M_REFRACTION under cast_ray); one where none has -- nothing is ever pushed (a scene on the M_REFRACTION forms for
 * their unbounded sums, pt_classify), at any depth */
static inline uint32_t pt_pend_entries(const PtSceneView &scene, uint32_t integrator, int32_t max_depth)
{
  const bool two_children = integrator == 1u ? scene.any_mirror_glass != 0u : scene.any_refract != 0u;
  return two_children ? (uint32_t)max_depth + 2u : 1u;
}
const char *pt_kernel_name_of(int which);
int pt_kernel_count(void);
unsigned long long pt_kernel_launches(int which);
uint32_t pt_pool_slots_per_xcd(bool park_pool); /* on the current device */
#ifdef PT_DEV_KERNELS
int pt_dev_variant();
#endif
hipError_t pt_launch_build_hull_flags(const double *tri_geom, const double *tri_normal, uint32_t n_tri, double tau,
                                      uint32_t *tri_object, hipStream_t stream);
hipError_t pt_launch_build_tables(const PtSceneView &scene, double near_R, float *filt, float *bvh_nodes, hipStream_t stream);
hipError_t pt_launch_selftest_xcc(unsigned int *counts, uint32_t n_workgroups, hipStream_t stream);
hipError_t pt_launch_selftest(int op, const double *a, const double *b, double *out, size_t n, hipStream_t stream);
hipError_t pt_launch_selftest_intersect(int kind, const double *rays, const double *prims, const double *entry_src,
                                        float *filt, float *tri32, uint32_t n, double near_R, double filt_shift,
                                        uint8_t *hit, double *tuv, unsigned long long *keep, hipStream_t stream);
/* the AOV kernels (pt_kernel.hip: render_aov, PT_AOV_FAMILY): which form a scene takes, the launch (a tile per wave; the outputs: PtAovOut),
 * names and launch counters (the scatter of their compact buffers to row-major images: pt_launch_untile_aov below) */
int pt_aov_pick(const PtSceneView &scene);
hipError_t pt_launch_aov(const PtLaunch &launch, const PtAovOut &out, hipStream_t stream, int which);
const char *pt_aov_kernel_name_of(int which);
int pt_aov_kernel_count(void);
unsigned long long pt_aov_kernel_launches(int which);
/* the ray-query kernels (pt_kernel.hip: query_rays, PT_QUERY_FAMILY): which form a scene takes, the launch (a ray per lane), names and
 * launch counters */
int pt_query_pick(const PtSceneView &scene);
hipError_t pt_launch_query(const PtLaunch &launch, const PtQuery &query, hipStream_t stream, int which);
const char *pt_query_kernel_name_of(int which);
int pt_query_kernel_count(void);
unsigned long long pt_query_kernel_launches(int which);
/* the sliced kernels (pt_kernel.hip: PT_SLICED_FAMILY, one table of two lists; body trace_sliced, pt_body_static.h): which of the
 * five forms a scene takes, in either list (as pt_query_pick), and per list the launch, names and launch counters.
 * The radiance queries (front end RayFront): 64 rays x 4 sample slices per workgroup; launch.samples, max_depth, seed, the
 * pending-ray pool and the status word as a render launch of the static M_REFRACTION members */
int pt_trace_pick(const PtSceneView &scene);
hipError_t pt_launch_trace(const PtLaunch &launch, const PtTrace &trace, hipStream_t stream, int which);
const char *pt_trace_kernel_name_of(int which);
int pt_trace_kernel_count(void);
unsigned long long pt_trace_kernel_launches(int which);
/* the pixel refinement (front end PixelFront): 64 entries x 4 sample slices per workgroup; what a radiance query's launch takes,
 * and the frame's size and camera */
hipError_t pt_launch_pixels(const PtLaunch &launch, const PtPixels &pixels, hipStream_t stream, int which);
const char *pt_pixel_kernel_name_of(int which);
int pt_pixel_kernel_count(void);
unsigned long long pt_pixel_kernel_launches(int which);
/* ---- the image-space passes (image_ops.hip, a translation unit of its own): launchers of kernels that see buffers of pixels or
 * of list entries and never a scene, a ray or a PtLaunch ---- */
/* the scatter of compact tile-major buffers to row-major images: the colour (floats and bytes, either may be null), and the AOV
 * kernels' 1- or 3-channel 32-bit buffers */
hipError_t pt_launch_untile(const float *tiles_rgb, const uint8_t *tiles_rgb8, int width, int height,
                            uint32_t tile_first, uint32_t tile_stride, uint32_t tile_count, float *image_rgb,
                            uint8_t *image_rgb8, hipStream_t stream);
hipError_t pt_launch_untile_aov(const uint32_t *tiles, uint32_t channels, int width, int height, uint32_t tile_first,
                                uint32_t tile_stride, uint32_t tile_count, uint32_t *image, hipStream_t stream);
/* the compaction: its workspace (the per-workgroup counts and every level of their scan; 0 for no pixel), and the launches on
 * `stream` -- the counts, the scan's levels (a loop over levels here on the host, no workgroup waits on another), the scatter
 * (capacity > 0 only).  *count gets the full count. */
size_t pt_select_workspace_bytes(uint64_t n);
hipError_t pt_launch_select(const PtSelect &args, void *workspace, uint32_t *indices, uint32_t capacity, uint32_t *count, hipStream_t stream);
/* the blend: one launch, an entry per lane */
hipError_t pt_launch_blend(const PtBlend &args, hipStream_t stream);
/* the denoiser: the prepare pass and `iterations` filter passes (the last one remodulates and tonemaps) on `stream` */
hipError_t pt_launch_denoise(const PtDenoise &args, int iterations, double sigma_color, hipStream_t stream);
/* temporal reprojection: one launch, a 16 x 16 block of pixels per workgroup, on `stream` */
hipError_t pt_launch_reproject(const PtReproject &args, hipStream_t stream);
/* the same from the caller's previous points (3 doubles per pixel) in place of step 3: pt_reproject_points */
hipError_t pt_launch_reproject_points(const PtReproject &args, const double *prev_points, hipStream_t stream);
/* the previous points of query hits: one launch, an entry per lane, on `stream` (n >= 1) */
hipError_t pt_launch_prev_points(const PtPrevPoints &args, hipStream_t stream);
hipError_t pt_launch_prev_points_moved(const PtPrevPointsMoved &args, hipStream_t stream);
/* guided upsampling: one launch, a 16 x 16 block of the high frame's pixels per workgroup, on `stream` */
hipError_t pt_launch_upsample(const PtUpsample &args, hipStream_t stream);
#endif

/* ---- the thin-lens camera (rt_hip.h, "thin-lens camera"; the kernels are lens.hip's, a translation unit of its own) ---- */
/* One sample pass's lens rays for the pixels [pixel_first, pixel_first + n) of a width-wide frame.  The camera as RtHipCamera
 * holds it; ax, ay: vec3_normalize of its horizontal and vertical, made on the host; w_minus_1 = (double)width - 1.0 and
 * h_minus_1 likewise (raytracer.c:203-204); lens_seed = rt_mix64(seed ^ 0x6C656E73); index_first = sample * NP + pixel_first,
 * the stream index of the first ray. */
struct PtLensRays
{
  double position[3], horizontal[3], vertical[3], lower_left_corner[3];
  double ax[3], ay[3];
  double w_minus_1, h_minus_1;
  double aperture_radius, focus_distance;
  uint64_t seed, lens_seed;
  uint32_t width, pixel_first, n, index_first;
  double *rays; /* n x 6 doubles, 16-byte aligned */
};

#define PT_LENS_ROUNDS 32 /* rejection rounds of the lens point before the centre is taken */

#if defined(__HIPCC__)
/* n >= 1 */
hipError_t lens_launch_rays(const PtLensRays &args, hipStream_t stream);
/* sum[3 * pixel_first + t] += radiance[t] for t < 3 n; a ray of status 2 makes its pixel's three sums NaN */
hipError_t lens_launch_accumulate(const uint32_t *status, const double *radiance, uint32_t pixel_first, uint32_t n, double *sum,
                                  hipStream_t stream);
/* mean = sum * (1.0 / samples) -> float and tonemapped byte, row-major; either output may be null */
hipError_t lens_launch_resolve(const double *sum, uint64_t n_pixels, int32_t samples, float *rgb, uint8_t *rgb8, hipStream_t stream);
#endif

/* ---- light probes (rt_hip.h, "light probes"; the kernels are probe.hip's, a translation unit of its own) ---- */
/* The contract's constants, here and nowhere else: the kernels and the shim read these. */
#define PT_PROBE_KEY 0x70726F62ull        /* the direction stream is (rt_mix64(seed ^ PT_PROBE_KEY), k, 0) */
#define PT_PROBE_ROUNDS 32                /* rejection rounds of a direction before (0, 0, 1) is taken */
#define PT_PROBE_Q_MIN 9.5367431640625e-07 /* 2^-20: a round whose squared length is below this is rejected */
#define PT_PROBE_Y0 0.28209479177387814
#define PT_PROBE_Y1 0.4886025119029199
#define PT_PROBE_Y2A 1.0925484305920792
#define PT_PROBE_Y2B 0.31539156525252005
#define PT_PROBE_Y2C 0.5462742152960396
#define PT_PROBE_K_SPHERE 12.566370614359172
#define PT_PROBE_K_HEMISPHERE 6.283185307179586
#define PT_PROBE_A0 3.141592653589793
#define PT_PROBE_A1 2.0943951023931953
#define PT_PROBE_A2 0.7853981633974483
#define PT_PROBE_SH 9 /* bases of a sphere probe; a hemisphere probe has one */

/* The probe rays of indices [k_first, k_first + n): ray k belongs to probe k / samples.  positions and normals hold 3 doubles a probe
 * (normals: hemisphere only); probe_seed = rt_mix64(seed ^ PT_PROBE_KEY); rays[0 .. 6) is ray k_first. */
struct PtProbeRays
{
  const double *positions, *normals;
  double *rays; /* n x 6 doubles, 16-byte aligned */
  uint64_t k_first, probe_seed;
  double bias;
  uint32_t n, samples, hemisphere;
};

/* One slice's fold: the slice holds the rays [k_first, k_first + n) -- their 6 doubles, status words and radiance --, and touches the
 * probes probe_first .. probe_first + n_probes - 1; sum holds bases x 3 doubles a probe (bases = hemisphere ? 1 : PT_PROBE_SH). */
struct PtProbeFold
{
  const double *rays, *radiance, *normals;
  const uint32_t *status;
  double *sum;
  uint32_t *probe_status; /* may be null */
  uint64_t k_first, probe_first, n_probes;
  uint32_t n, samples, hemisphere;
};

#if defined(__HIPCC__)
/* n >= 1 */
hipError_t probe_launch_rays(const PtProbeRays &args, hipStream_t stream);
/* n >= 1: sum = sum + (radiance * w) over the slice's rays of each probe in ascending k, a thread a (probe, basis, channel); a ray
 * of status 2 makes its probe's sums NaN and its probe_status 2 */
hipError_t probe_launch_fold(const PtProbeFold &args, hipStream_t stream);
/* coeff = (sum * (1.0 / samples)) * k for n_values values; coeff_f (may be null) = (float)coeff */
hipError_t probe_launch_resolve(const double *sum, uint64_t n_values, int32_t samples, double k, double *coeff, float *coeff_f,
                                hipStream_t stream);
/* m >= 1 entries (probe index, normal): the irradiance of rt_hip.h from n_probes x PT_PROBE_SH x 3 coefficients, 3 doubles an entry */
hipError_t probe_launch_irradiance(const double *coeff, uint64_t n_probes, const uint32_t *index, const double *normals, uint64_t m,
                                   double *irradiance, hipStream_t stream);
#endif

/* ---- probe grids (rt_hip.h, "probe grids"; the kernels are probe.hip's) ---- */
#define PT_GRID_FACING 1u              /* RT_HIP_GRID_FACING */
#define PT_GRID_FACE_FLOOR 0.2         /* face = s*s + PT_GRID_FACE_FLOOR */
#define PT_GRID_INV_PI 0.3183098861837907 /* a Lambertian surface's radiance is albedo * E * (1 / pi) */

/* A checked RtHipProbeGrid as the kernels take it */
struct PtGrid
{
  double origin[3], step[3];
  uint32_t count[3], flags;
  float miss_color[3];
};

/* m entries shaded from the grid's n x PT_PROBE_SH x 3 coefficients; status, albedo and add may be null, irradiance or color too
 * (not both) */
struct PtProbeShade
{
  PtGrid grid;
  const double *coeff, *points, *normals;
  const uint32_t *status;
  const float *albedo, *add;
  double *irradiance;
  float *color;
  uint32_t m;
};

#if defined(__HIPCC__)
/* the grid's n x 3 positions, a thread a probe */
hipError_t probe_launch_grid_positions(const PtGrid &grid, double *positions, hipStream_t stream);
/* m >= 1: rt_hip.h's probe shade, a thread an entry */
hipError_t probe_launch_shade(const PtProbeShade &args, hipStream_t stream);
/* add[3 i + c] = (float)emission[stride * object[i] + c] for object[i] < n_objects, else +0.0f: n entries, emission a table of
 * n_objects records of `stride` doubles */
hipError_t probe_launch_emission(const uint32_t *object, uint64_t n, const double *emission, uint32_t stride, uint32_t n_objects, float *add,
                                 hipStream_t stream);
/* rgb8 = pt_math.h's tonemap of (double)rgb, n_values values */
hipError_t probe_launch_tonemap(const float *rgb, uint64_t n_values, uint8_t *rgb8, hipStream_t stream);
/* uv[2 p] = ((double)x + 0.5) / ((double)width - 1.0), uv[2 p + 1] = ((double)y + 0.5) / ((double)height - 1.0), p = y * width + x */
hipError_t probe_launch_pixel_centres(uint32_t width, uint32_t height, double *uv, hipStream_t stream);
#endif

/* ---- probe visibility (rt_hip.h, "probe visibility"; the kernels are probe.hip's) ---- */
#define PT_VIS_RES_MIN 2u
#define PT_VIS_RES_MAX 32u
#define PT_VIS_SHARP_MAX 8u

/* A checked RtHipProbeVis as the kernels take it */
struct PtProbeVis
{
  double d_max, bias, floor;
  uint32_t res, sharp;
};

/* One slice's depth fold: the slice holds the rays [k_first, k_first + n) -- their 6 doubles, the query's status words and t --, and
 * touches the probes probe_first .. probe_first + n_probes - 1; sum holds res x res x 3 doubles a probe: (W, M1, M2) a texel. */
struct PtProbeDepthFold
{
  const double *rays, *t;
  const uint32_t *status;
  double *sum;
  uint32_t *probe_status; /* may be null */
  uint64_t k_first, probe_first, n_probes;
  uint32_t n, samples;
  PtProbeVis vis;
};

/* the shade's arguments and the moments: n x res x res x 2 doubles (mean, mean2) */
struct PtProbeShadeVis
{
  PtProbeShade shade;
  PtProbeVis vis;
  const double *moments;
};

#if defined(__HIPCC__)
/* n >= 1: (W, M1, M2) of each (probe, texel) over the slice's rays of the probe in ascending k, a thread a (probe, texel); a ray of
 * status 2 makes its probe's sums NaN and its probe_status 2 */
hipError_t probe_launch_depth_fold(const PtProbeDepthFold &args, hipStream_t stream);
/* moments[2 i] = W > 0 ? M1 / W : d_max, moments[2 i + 1] = W > 0 ? M2 / W : d_max * d_max for n_texels (probe, texel) pairs */
hipError_t probe_launch_depth_resolve(const double *sum, uint64_t n_texels, double d_max, double *moments, hipStream_t stream);
/* m >= 1: rt_hip.h's probe shade with the visibility weight, a thread an entry */
hipError_t probe_launch_shade_vis(const PtProbeShadeVis &args, hipStream_t stream);
#endif

/* ---- probe updates (rt_hip.h, "probe updates"; the kernels are probe.hip's) ---- */

/* A round's probes: i_j = phase + j * stride for j = 0 .. m - 1, every one below the grid's count */
struct PtProbeRound
{
  uint32_t stride, phase, m;
};

/* the coefficient blend of a round: sum holds m x PT_PROBE_SH x 3 doubles by j; coeff, coeff_f, change and age are the grid's, by i;
 * coeff_f and change_out may be null */
struct PtProbeCoeffBlend
{
  PtProbeRound round;
  const double *sum;
  const uint32_t *age;
  double *coeff;
  float *coeff_f;
  double *change_out;
  double inv_samples, k, hysteresis, change, fast;
};

/* the moment blend of a round: sums holds m x res x res x 3 doubles (W, M1, M2) by j; moments the grid's res x res x 2 a probe, by i */
struct PtProbeMomentBlend
{
  PtProbeRound round;
  const double *sums;
  const uint32_t *age;
  double *moments;
  double hysteresis, d_max;
  uint32_t res;
};

#if defined(__HIPCC__)
/* m >= 1: positions[3 j ..] = the grid's position of probe i_j, a thread an updated probe */
hipError_t probe_launch_grid_positions_strided(const PtGrid &grid, const PtProbeRound &round, double *positions, hipStream_t stream);
/* m >= 1: rt_hip.h's coefficient blend, a thread an (updated probe, basis, channel) */
hipError_t probe_launch_coeff_blend(const PtProbeCoeffBlend &args, hipStream_t stream);
/* m >= 1: rt_hip.h's moment blend, a thread an (updated probe, texel) */
hipError_t probe_launch_moment_blend(const PtProbeMomentBlend &args, hipStream_t stream);
/* m >= 1: age[i_j] steps up to 0xFFFFFFFF and stays; where both are given, status[i_j] = round_status[j] */
hipError_t probe_launch_age_step(const PtProbeRound &round, uint32_t *age, const uint32_t *round_status, uint32_t *status, hipStream_t stream);
#endif


#endif /* PT_DEVICE_H */

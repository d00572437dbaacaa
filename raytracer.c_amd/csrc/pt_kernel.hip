/* pt_kernel.hip -- the path-tracing hot path, hand-written for gfx950 (CDNA4).
 *
 * Replaces, per pixel, the loop nest of the reference's render()
 * (gue-ni/raytracer.c raytracer.c:184-222) and everything it reaches:
 * get_camera_ray :375-384, trace_path :482-554 (the recursion rewritten as an
 * iterative bounce loop carrying a throughput), intersect :393-464,
 * intersect_sphere :77-118, intersect_triangle :120-174, the RNG helpers
 * :227-253, reflect :349-352, checkered_texture :386-391, the sample mean and
 * gamma-5 tonemap :212-220.
 *
 * pt_render_tiles (shipped).  One workgroup = one 8x8 pixel tile = 4 wavefronts;
 * wavefront w owns tile rows 2w, 2w+1 (16 pixels) and their 16*spp samples as a POOL of
 * jobs.  Each lane runs a flattened state machine: one loop iteration = one
 * trace_path() call of the reference; a lane whose path ends adds its sample to the
 * pixel's accumulator and pulls the next (pixel, sample) job of the pool in the same
 * iteration slot (wave-synchronous: ballot + prefix count, no atomics), so all 64 lanes
 * stay busy until the pool is dry whatever the individual path lengths are.  The scene
 * scan -- 80 % of the work -- is split into a wave-uniform conservative filter and a
 * per-lane exact test over the survivors (scan_filtered below).  Per-pixel sums are
 * kept in LDS as 64-bit FIXED-POINT integers (power-of-two scale chosen per launch from a
 * bound on the radiance, ~2^-40 relative resolution): integer addition is associative,
 * so the image is bit-identical under any lane / tile / GPU assignment although samples
 * finish in a data-dependent order.  The tile leaves as one coalesced 768-byte float3
 * store (+192 tonemapped bytes).
 *   Three more things keep lanes from idling in divergent code (render_tiles_pooled):
 * camera samples are prepared 64 at a time by the whole wave into an LDS queue instead of by
 * whichever few lanes are idle; the direction of a diffuse hit gets four rejection rounds per
 * trip and the rare lane still without a sample carries on next trip instead of the wave
 * looping on it; and, in scenes with a triangle hierarchy, rays that can reach the mesh wait
 * until a batch of them walks it together.  None of this can change a value: a sample
 * depends only on its (seed, pixel, sample) stream.
 *
 * Kernel family: pt_render_tiles[_tri][_big][_chk] (pooled body, by scene content), pt_render_tiles_pool_mem* (the same body
 * with geometry read from memory: scenes beyond the LDS staging budget, and sphere scenes beyond ~85 spheres by preference),
 * pt_render_tiles_refr_pool (the same body for small sphere scenes with M_REFRACTION: windowed pixel sums, pending rays that
 * travel with a path), pt_render_tiles_tri_queued* (hierarchy scenes: parked walks; _refr: with M_REFRACTION), pt_render_tiles[..]_refr and
 * pt_whitted_tiles[..] (static body: refraction's two-child tree where the pooled kernel does not apply, and cast_ray,
 * raytracer.c:556-641): one list, PT_FAMILY below; which member a launch takes: pt_pick_kernel, inside pt_plan_launch.
 *
 * pt_render_tiles_v0 (development builds only, -DPT_DEV_KERNELS: kept for A/B and as the plainest statement of the algorithm): static
 * assignment lane = (pixel, sample slice), literal scan, fp64 partial sums combined by
 * xor-shuffles in a fixed order.
 *
 * Numerics: everything on the decision path (hit / miss, closest index, Russian
 * roulette, rejection sampling, hemisphere flip) is fp64 in exactly the reference's
 * operation order, compiled with -ffp-contract=off, IEEE sqrt and division -- so every
 * branch decision, hence every RNG draw and the ray / test counters, equals the CPU
 * reference's bit for bit.  Only the radiance VALUE is accumulated differently (forward:
 * L += T*e; T *= albedo*cos instead of the recursive nesting; fixed-point sample sum), a
 * ~1e-12 relative difference, far inside the float32 output's rounding.
 *
 * No MFMA: branchy fp64 scalar-per-lane math with no dense contraction.  The bounding
 * roof is the fp64 VALU issue rate.
 *
 * Layout.  The path tracer's device code is ONE translation unit -- every body is a template instantiated below, and the kernels
 * share their inlined pieces -- split by topic into headers that are included here, in this order, and (but for pt_math.h, which
 * lens.hip and image_ops.hip take as well) nowhere else:
 *   pt_math.h         vectors, RNG draws, fixed-point terms, tonemap, tile_pixel, atan2_tab / cube / frac1, PT_DIAG / PT_PHASE macros
 *   pt_intersect.h    exact_sphere / exact_triangle (fp64, the reference's operation order), the hierarchy in packed fp32
 *   pt_filter.h       the phase-1 filter (three forms), BigPrune, tile_cull, the fp32 triangle pre-test, scan_filtered
 *   pt_scene_ctx.h    SceneCtx / stage_scene, intersect_scene (scan_filtered over a SceneCtx, callers without a TriLast), Path, pending-ray stacks, windowed sums, camera, start_sample
 *   pt_trace.h        trace_step (trace_path), whitted_step (cast_ray), finish_pixels / store_tile_pixels / store_tile
 *   pt_body_pooled.h  render_tiles_pooled   (pt_render_tiles[_tri][_big][_chk], _pool_mem*, _refr_pool*)
 *   pt_body_queued.h  render_tiles_queued   (pt_render_tiles_tri_queued*: parked walks, also with M_REFRACTION)
 *   pt_body_static.h  render_tiles_static   (pt_render_tiles_v0, *_refr, pt_whitted_tiles*, *_mem)
 *                     trace_sliced          (pt_trace_rays*, pt_trace_pixels*), pend_acquire, reduce_slices
 * This file keeps the kernel family (PT_FAMILY: the entry points, their ids and properties), the AOV kernels (render_aov,
 * PT_AOV_FAMILY: first-hit feature buffers, not members of the family), the ray-query kernels (query_rays, PT_QUERY_FAMILY: closest
 * hits of the caller's rays, a list of their own too), the sliced kernels (PT_SLICED_FAMILY: trace_sliced behind the front ends
 * RayFront -- trace_path along the caller's rays -- and PixelFront -- the render's samples of listed pixels --, one table of two
 * more such lists), the resolves and the adaptive sampler's tile kernels (they read a PtLaunch or tile sample counts), the
 * table-building and self-test kernels,
 * and the host side declared in pt_device.h: the launch plan (pt_plan_launch, around the pick table pt_pick_kernel) and the
 * launchers (pt_launch_render, pt_launch_aov, pt_launch_query, pt_launch_trace, pt_launch_pixels).  The five lists are a
 * PtKernelList each (rows + launch counters) and the five launchers go through launch_staged (dynamic-LDS limit, launch, error).
 * The kernels that see neither a scene nor a ray nor a PtLaunch -- untile, denoise, reproject, previous points, upsample, select,
 * blend -- are image_ops.hip, a translation unit of its own, as bvh_device.hip, scene_update.hip and lens.hip are.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <atomic>

#include "pt_device.h"
#include "rt_rng.h"

#include "pt_math.h"
#include "pt_intersect.h"
#include "pt_filter.h"
#include "pt_scene_ctx.h"
#include "pt_trace.h"
#include "pt_body_pooled.h"
#include "pt_body_queued.h"
#include "pt_body_static.h"

/* ---- the kernel family: ONE list, one line per member ----------------------------------------------------------------------
 * Each line gives the member's id (what pt_pick_table names), its entry point, its __launch_bounds__, its properties and the
 * body it instantiates.  The entry points, the ids (enum PtKernelId) and the rows of pt_kernels[] are all generated from it, in
 * this order: rt_hip_kernel_launches(index) and the coverage table list the members in it.
 *
 * Names, by scene content (pt_pick_kernel): pt_render_tiles[_tri][_big][_chk|_refr]: "_tri" = scene has triangles; "_big" = the
 * filter table is not in LDS (more than PT_FILT_LDS_MAX primitives, or centres / radii beyond fp32's comfortable range): table by
 * scalar loads, NaN-safe compares, triangles through the hierarchy; "_chk" = scene has M_CHECKERED materials (atan2_tab / frac1);
 * "_refr" = scene has M_REFRACTION materials (static body + pending second children in the pool; also covers M_CHECKERED).
 * pt_render_tiles itself is the headline configuration: diffuse / mirror / emissive spheres, small scene.
 *   pt_render_tiles_tri_queued*   hierarchy scenes with parked walks (_sph: round meshes, the probe is the triangles' bounding
 *                                 sphere alone; _refr: with M_REFRACTION -- windowed sums in the workspace, pending second children
 *                                 that travel with a path, also through the ring; _mem: spheres beyond the LDS staging budget next
 *                                 to such a mesh, sphere geometry, materials and filter pairs from memory, the general probe).  The
 *                                 pooled _tri / _tri_big kernels are the table's park = NO rows (no ring workspace, or a scene beyond
 *                                 fp32's comfortable range) and RT_HIP_KERNEL_VARIANT=2 of the development build for A/B.  (No
 *                                 _mem refraction form: at three waves it spills two doubles inside the trip loop, and scenes with
 *                                 M_REFRACTION, more spheres than the staging holds AND a large mesh are the rarest class there is
 *                                 -- they keep pt_render_tiles_mem.)
 *   pt_render_tiles_*refr_pool*   M_REFRACTION on the pooled body: small sphere scenes, streamed sphere scenes (_mem: the
 *                                 reference's own generator gives a fifth of its spheres M_REFRACTION, main.c:107-115, so a large
 *                                 packed room is exactly this class), small scenes with a mesh (_tri).
 *   pt_render_tiles_pool_mem*     scenes whose sphere geometry + materials exceed the LDS staging budget (pt_geom_in_lds: more than
 *                                 256 spheres): the SAME pooled body -- job pool, swap, fixed-point sums, four rejection rounds per
 *                                 trip, sample chunks -- with geometry and materials gathered from memory (PtSceneView.geom4 /
 *                                 material: 32 + 64 bytes per sphere, L2-resident up to tens of thousands of spheres) and the filter
 *                                 table streamed through scalar loads as in the _big kernels.  _s: sphere-only scenes within fp32's
 *                                 comfortable range, with the small scenes' FORM of the filter -- sign tests, per-tile culling of
 *                                 the primary trips, the walls pruned among themselves -- read from memory (stage_scene,
 *                                 FILT_FROM_MEMORY); measured on rooms packed as main.c:65-138 would (tools/many_spheres.py,
 *                                 profiles/r04_many_spheres.txt).  Until round 4 the 257th sphere dropped a scene onto
 *                                 pt_render_tiles_mem, the static body with every material's code and a 2.7 KB private stack per lane.
 *   pt_whitted_tiles[..]          cast_ray (raytracer.c:556-641): the static body with whitted_step, without a pending-ray stack
 *                                 (scenes with a material that has both M_REFLECTION and M_REFRACTION take pt_whitted_tiles_mem).
 *   pt_render_tiles_mem, pt_whitted_tiles_mem   beyond the staging budget (more than ~256 spheres, or thousands of meshes): the most
 *                                 general static body -- every material, triangles through the hierarchy -- reading geometry and
 *                                 materials from memory.  The O(n) sphere scan dominates such scenes whatever the kernel around it does.
 *
 * Properties (PtKernelProps), by name:
 *   PEND_POOL    pushes pending second children: needs a slot of the pending-ray pool (rt_hip_shim.hip, pend_pool_for)
 *   QUEUED       parked walks: a tile per WAVE (four work units per workgroup), filter pairs + traversal stacks in dynamic LDS
 *   STAGES_NONE  geometry and tables from memory: no staged scene in LDS, whatever the scene's size
 *   WIDE_PEND    4 x 512 stacks per pool slot (path ids that travel through the ring)
 *   CHUNKS       takes sample_chunks > 1 (integer partial sums merged by pt_resolve_tiles)
 *   WINDOWED     ... as windowed sums (win_add): PT_ACC_WS_WORDS_WIN words per tile of the chunk workspace
 *   MIXED        takes a mixed grid (PtLaunch.n_whole > 0): whole tiles, then the last tiles as sample chunks, in one launch */
enum PtKernelProps : uint32_t
{
  PEND_POOL = 1u, QUEUED = 2u, STAGES_NONE = 4u, WIDE_PEND = 8u, CHUNKS = 16u, WINDOWED = 32u, MIXED = 64u
};

/* launch bounds (waves per SIMD; PT_MIN_WAVES, _TRI, _CHK: pt_body_pooled.h).  `make variant DEFS=-DPT_MIN_WAVES_...` and
 * tools/gpu_ab.py override them.  _tri_big: 24 KB of traversal stacks, 4 workgroups per CU. */
#ifndef PT_MIN_WAVES_QUEUED
#define PT_MIN_WAVES_QUEUED 4
#endif
#ifndef PT_MIN_WAVES_QUEUED_REFR
#define PT_MIN_WAVES_QUEUED_REFR 3
#endif
#ifndef PT_MIN_WAVES_REFR_POOL
#define PT_MIN_WAVES_REFR_POOL 4
#endif
/* the static M_REFRACTION kernels.  Until round 4 they had none: 203-232 VGPRs and a 2.7 KB private stack, two waves per SIMD.
 * With the pending rays in the pool (PendStack) and the material code's library calls gone (atan2_tab, cube, frac1) the sphere
 * kernels need 127 VGPRs and the mesh kernels ~150, without scratch */
#ifndef PT_MIN_WAVES_REFR
#define PT_MIN_WAVES_REFR 4
#endif
#ifndef PT_MIN_WAVES_REFR_TRI
#define PT_MIN_WAVES_REFR_TRI 3
#endif
/* cast_ray, measured on the MI355X (1920x1080 x 64 spp, ms at 4 / 3 / 2 waves per SIMD): spheres (config 4) 8.2 / 8.4 / 9.4;
 * small mesh (config 3) 6.2 / 5.2 / 6.5; hierarchy (config 5, 4K x 8 spp) 8.6 / 8.1 / 8.9.  None of the three is free of
 * scratch below 2 waves (228-308 B at 4, 44-156 B at 3). */
#ifndef PT_MIN_WAVES_WHITTED
#define PT_MIN_WAVES_WHITTED 4
#endif
#ifndef PT_MIN_WAVES_WHITTED_TRI
#define PT_MIN_WAVES_WHITTED_TRI 3
#endif

/* bodies: render_tiles_pooled<CHECKER, TRIS, FILT_LDS, GEOM_LDS[, REFR]>, render_tiles_queued<CHECKER[, SPHERE_PROBE, REFR,
 * GEOM_LDS]>, render_tiles_static<VARIANT, REFRACT, CHECKER, TRIS, FILT_LDS, WHITTED, GEOM_LDS> */
#define PT_FAMILY(X) \
  X(K_TILES,               pt_render_tiles,                     (PT_BLOCK, PT_MIN_WAVES),             CHUNKS | MIXED,                                     render_tiles_pooled<false, false, true, true, false, true>) \
  X(K_BIG,                 pt_render_tiles_big,                 (PT_BLOCK, PT_MIN_WAVES),             CHUNKS,                                             render_tiles_pooled<false, false, false, true>) \
  X(K_TRI,                 pt_render_tiles_tri,                 (PT_BLOCK, PT_MIN_WAVES_TRI),         CHUNKS,                                             render_tiles_pooled<false, true, true, true>) \
  X(K_TRI_BIG,             pt_render_tiles_tri_big,             (PT_BLOCK, 4),                        CHUNKS,                                             render_tiles_pooled<false, true, false, true>) \
  X(K_CHK,                 pt_render_tiles_chk,                 (PT_BLOCK, PT_MIN_WAVES_CHK),         CHUNKS,                                             render_tiles_pooled<true, false, true, true>) \
  X(K_BIG_CHK,             pt_render_tiles_big_chk,             (PT_BLOCK, PT_MIN_WAVES_CHK),         CHUNKS,                                             render_tiles_pooled<true, false, false, true>) \
  X(K_TRI_CHK,             pt_render_tiles_tri_chk,             (PT_BLOCK),                           CHUNKS,                                             render_tiles_pooled<true, true, true, true>) \
  X(K_TRI_BIG_CHK,         pt_render_tiles_tri_big_chk,         (PT_BLOCK),                           CHUNKS,                                             render_tiles_pooled<true, true, false, true>) \
  X(K_REFR,                pt_render_tiles_refr,                (PT_BLOCK, PT_MIN_WAVES_REFR),        PEND_POOL,                                          render_tiles_static<1, true, true, false, true, 0, true>) \
  X(K_BIG_REFR,            pt_render_tiles_big_refr,            (PT_BLOCK, PT_MIN_WAVES_REFR),        PEND_POOL,                                          render_tiles_static<1, true, true, false, false, 0, true>) \
  X(K_TRI_REFR,            pt_render_tiles_tri_refr,            (PT_BLOCK, PT_MIN_WAVES_REFR_TRI),    PEND_POOL,                                          render_tiles_static<1, true, true, true, true, 0, true>) \
  X(K_TRI_BIG_REFR,        pt_render_tiles_tri_big_refr,        (PT_BLOCK, PT_MIN_WAVES_REFR_TRI),    PEND_POOL,                                          render_tiles_static<1, true, true, true, false, 0, true>) \
  X(K_WHITTED,             pt_whitted_tiles,                    (PT_BLOCK, PT_MIN_WAVES_WHITTED),     0,                                                  render_tiles_static<1, false, true, false, true, 1, true>) \
  X(K_WHITTED_BIG,         pt_whitted_tiles_big,                (PT_BLOCK, PT_MIN_WAVES_WHITTED),     0,                                                  render_tiles_static<1, false, true, false, false, 1, true>) \
  X(K_WHITTED_TRI,         pt_whitted_tiles_tri,                (PT_BLOCK, PT_MIN_WAVES_WHITTED_TRI), 0,                                                  render_tiles_static<1, false, true, true, true, 1, true>) \
  X(K_WHITTED_TRI_BIG,     pt_whitted_tiles_tri_big,            (PT_BLOCK, PT_MIN_WAVES_WHITTED_TRI), 0,                                                  render_tiles_static<1, false, true, true, false, 1, true>) \
  X(K_MEM,                 pt_render_tiles_mem,                 (PT_BLOCK),                           PEND_POOL,                                          render_tiles_static<1, true, true, true, false, 0, false>) \
  X(K_WHITTED_MEM,         pt_whitted_tiles_mem,                (PT_BLOCK),                           PEND_POOL,                                          render_tiles_static<1, false, true, true, false, 2, false>) \
  X(K_TRI_QUEUED,          pt_render_tiles_tri_queued,          (PT_BLOCK, PT_MIN_WAVES_QUEUED),      QUEUED | CHUNKS,                                    render_tiles_queued<false>) \
  X(K_TRI_QUEUED_CHK,      pt_render_tiles_tri_queued_chk,      (PT_BLOCK),                           QUEUED | CHUNKS,                                    render_tiles_queued<true>) \
  X(K_TRI_QUEUED_SPH,      pt_render_tiles_tri_queued_sph,      (PT_BLOCK, PT_MIN_WAVES_QUEUED),      QUEUED | CHUNKS,                                    render_tiles_queued<false, true>) \
  X(K_POOL_MEM,            pt_render_tiles_pool_mem,            (PT_BLOCK, PT_MIN_WAVES),             STAGES_NONE | CHUNKS,                               render_tiles_pooled<false, false, false, false>) \
  X(K_POOL_MEM_CHK,        pt_render_tiles_pool_mem_chk,        (PT_BLOCK),                           STAGES_NONE | CHUNKS,                               render_tiles_pooled<true, false, false, false>) \
  X(K_POOL_MEM_TRI,        pt_render_tiles_pool_mem_tri,        (PT_BLOCK, 4),                        STAGES_NONE | CHUNKS,                               render_tiles_pooled<false, true, false, false>) \
  X(K_POOL_MEM_TRI_CHK,    pt_render_tiles_pool_mem_tri_chk,    (PT_BLOCK),                           STAGES_NONE | CHUNKS,                               render_tiles_pooled<true, true, false, false>) \
  X(K_POOL_MEM_S,          pt_render_tiles_pool_mem_s,          (PT_BLOCK, PT_MIN_WAVES),             STAGES_NONE | CHUNKS,                               render_tiles_pooled<false, false, true, false>) \
  X(K_POOL_MEM_S_CHK,      pt_render_tiles_pool_mem_s_chk,      (PT_BLOCK),                           STAGES_NONE | CHUNKS,                               render_tiles_pooled<true, false, true, false>) \
  X(K_REFR_POOL,           pt_render_tiles_refr_pool,           (PT_BLOCK, PT_MIN_WAVES_REFR_POOL),   PEND_POOL | CHUNKS | WINDOWED,                      render_tiles_pooled<true, false, true, true, true>) \
  X(K_REFR_POOL_MEM,       pt_render_tiles_refr_pool_mem,       (PT_BLOCK, PT_MIN_WAVES_REFR_POOL),   PEND_POOL | STAGES_NONE | CHUNKS | WINDOWED,        render_tiles_pooled<true, false, true, false, true>) \
  X(K_TRI_REFR_POOL,       pt_render_tiles_tri_refr_pool,       (PT_BLOCK, 3),                        PEND_POOL | CHUNKS | WINDOWED,                      render_tiles_pooled<true, true, true, true, true>) \
  X(K_TRI_QUEUED_REFR,     pt_render_tiles_tri_queued_refr,     (PT_BLOCK, PT_MIN_WAVES_QUEUED_REFR), PEND_POOL | QUEUED | WIDE_PEND | CHUNKS | WINDOWED, render_tiles_queued<true, false, true>) \
  X(K_TRI_QUEUED_REFR_SPH, pt_render_tiles_tri_queued_refr_sph, (PT_BLOCK, PT_MIN_WAVES_QUEUED_REFR), PEND_POOL | QUEUED | WIDE_PEND | CHUNKS | WINDOWED, render_tiles_queued<true, true, true>) \
  X(K_TRI_QUEUED_CHK_SPH,  pt_render_tiles_tri_queued_chk_sph,  (PT_BLOCK),                           QUEUED | CHUNKS,                                    render_tiles_queued<true, true>) \
  X(K_TRI_QUEUED_MEM,      pt_render_tiles_tri_queued_mem,      (PT_BLOCK, PT_MIN_WAVES_QUEUED),      QUEUED | STAGES_NONE | CHUNKS,                      render_tiles_queued<false, false, false, false>) \
  X(K_TRI_QUEUED_MEM_CHK,  pt_render_tiles_tri_queued_mem_chk,  (PT_BLOCK),                           QUEUED | STAGES_NONE | CHUNKS,                      render_tiles_queued<true, false, false, false>)
/* the literal single-phase scan: development builds only (RT_HIP_KERNEL_VARIANT=0), the last member */
#ifdef PT_DEV_KERNELS
#define PT_FAMILY_DEV(X) X(K_V0, pt_render_tiles_v0, (PT_BLOCK), 0, render_tiles_static<0, false, true, true, false, 0, true>)
#else
#define PT_FAMILY_DEV(X)
#endif

#define PT_ENTRY(id, name, bounds, props, ...) \
  extern "C" __global__ __launch_bounds__ bounds void name(const PtLaunch L) { __VA_ARGS__(L, false); } \
  extern "C" __global__ __launch_bounds__ bounds void name##_list(const PtLaunch L) { __VA_ARGS__(L, true); }
PT_FAMILY(PT_ENTRY)
PT_FAMILY_DEV(PT_ENTRY)
#undef PT_ENTRY

/* ---- a kernel list on the host: the rows an X-macro list generates, and how often each was launched in this process
 * (what a test run actually exercised).  The five lists (PT_FAMILY, PT_AOV_FAMILY, PT_QUERY_FAMILY and the two columns of PT_SLICED_FAMILY) are one of these each;
 * pt_*_name_of / _count / _launches (pt_device.h) ask it.  The lists' ids come from PT_LIST_ID, the rows of the two plain
 * lists from PT_LIST_INFO; the family's rows carry more (PT_INFO), and each list's entry points have their own signature, so
 * the three ENTRY macros stay apart. */
template <class Info, int N>
struct PtKernelList
{
  Info info[N];
  std::atomic<unsigned long long> counts[N];
  bool valid(int i) const { return i >= 0 && i < N; }
  const Info &operator[](int i) const { return info[i]; }
  const char *name_of(int i) const { return valid(i) ? info[i].name : ""; }
  unsigned long long launches(int i) const { return valid(i) ? counts[i].load() : 0ull; }
  void launched(int i) { counts[i].fetch_add(1ull); }
};
/* a row of a list without properties (the AOV and the ray-query kernels) */
template <class Fn>
struct PtEntryInfo
{
  const char *name;
  Fn fn;
};
#define PT_LIST_ID(id, ...) id,
#define PT_LIST_INFO(id, name, ...) {#name, name},

enum PtKernelId
{
  PT_FAMILY(PT_LIST_ID) PT_FAMILY_DEV(PT_LIST_ID) K_COUNT
};
typedef void (*PtKernelFn)(const PtLaunch);
struct PtKernelInfo
{
  const char *name;
  PtKernelFn fn;
  PtKernelFn fn_list; /* the same member over a slot list (PtLaunch.slot_list): the passes of an accumulation with frozen tiles */
  uint32_t props; /* PtKernelProps */
  bool has(uint32_t p) const { return (props & p) != 0u; }
  uint32_t pend_columns() const { return has(WIDE_PEND) ? 4u * 512u : PT_PEND_COLUMNS; }
};
#define PT_INFO(id, name, bounds, props, ...) {#name, name, name##_list, props},
static PtKernelList<PtKernelInfo, K_COUNT> pt_kernels = {{PT_FAMILY(PT_INFO) PT_FAMILY_DEV(PT_INFO)}};
#undef PT_INFO

/* ---- AOV body: a workgroup = four tiles, a wave = one tile, a lane = one pixel ----------------------------------------------
 * A lane runs the pixel's samples s = 0 .. samples - 1 in ascending order.  Per sample: the camera ray of beauty sample s
 * (start_sample: the first two draws of the (seed, pixel, s) stream, get_camera_ray), then ONE intersect() -- scan_filtered,
 * the exact-test path of the beauty kernels with the same filter, pre-tests, hierarchy and TriLast rule, so the first hit is
 * theirs by construction -- and from the winner what trace_path's first call forms: the unit normal (never flipped), the
 * object's colour as given (not divided by the roulette probability) or its checkered_texture, and t.  A miss counts as
 * BACKGROUND albedo and a zero normal.  The sums are fp64 vec3_add in sample order from zero, scaled by 1.0 / samples and
 * rounded to float32 (render(), raytracer.c:199-215): the lane holds its pixel's sums alone, so there is no cross-lane
 * reduction and the order is the contract's.  No path state, no pool, no ring, no status word: nothing can run out.
 * CHECKER: the scene has M_CHECKERED materials (u, v tracked); TRIS: triangles (flat scan with FILT_LDS, else the hierarchy);
 * FILT_LDS: the filter table is staged (pt_filter_in_lds); GEOM_LDS: sphere geometry + materials are staged (pt_geom_in_lds). */
template <bool CHECKER, bool TRIS, bool FILT_LDS, bool GEOM_LDS>
__device__ __forceinline__ void render_aov(const PtLaunch &L, const PtAovOut &O)
{
  static_assert(GEOM_LDS || !FILT_LDS, "a staged filter table comes with staged geometry");
  extern __shared__ __attribute__((aligned(16))) double lds[];
  SceneCtx S_init = stage_scene<GEOM_LDS, FILT_LDS>(L, lds);
  __shared__ double atan_tab[CHECKER ? PT_ATAN_TAB : 1];
  if (CHECKER)
  {
    atan_table_to_lds(atan_tab);
    S_init.atan_tab = atan_tab;
  }
  const SceneCtx S = S_init;
  __syncthreads();

  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t slot = blockIdx.x * (PT_BLOCK / 64u) + wave;
  if (slot >= L.tile_count)
    return; /* the last workgroup's spare waves (no barrier follows) */
  const uint32_t tile = L.tile_first + slot * L.tile_stride;
  uint32_t px, py;
  const bool inside = tile_pixel(L.tiles_x, tile, lane, L.width, L.height, px, py);
  const uint32_t pixel = py * (uint32_t)L.width + px;
  const uint64_t pixel_key = rt_rng_pixel_key(L.seed, pixel);
  const CameraRegs cam = load_camera(L);
  constexpr bool BVH = TRIS && !FILT_LDS;
  constexpr bool LAST = CHECKER && TRIS;

  V3 alb_sum = {0, 0, 0}, nrm_sum = {0, 0, 0};
  double t_min = __longlong_as_double(0x7FF0000000000000ll); /* +inf: no sample hit yet */
  uint32_t object = 0xFFFFFFFFu, hits = 0u;
  const uint32_t spp = inside ? (uint32_t)L.samples : 0u;
  for (uint32_t s = 0; s < spp; s++)
  {
    Path P;
    start_sample(P, cam, pixel_key, px, py, sample_term(s));
    const V3 o = P.o, d = P.d;
    double min_t = S.t_start, bary_u = 0, bary_v = 0;
    int best = -1;
    TriLast last = {-1, 0, 0};
    /* trace_step's intersect() call, argument for argument (VARIANT 1, MODE 0) */
    scan_filtered<TRIS, BVH, FILT_LDS, true, LAST>(
        S.geom, S.tri, FILT_LDS ? S.filt_lds : S.filt, S.near_R2, S.n_sph, S.n_sph + S.n_tri, o, d, min_t, best, bary_u, bary_v,
        nullptr, S.bvh_nodes, S.n_bvh_nodes, S.bvh_tri, S.filt_shift, &last, S.stale_uv, S.tri32, nullptr, S.big,
        (TRIS && FILT_LDS && !LAST) ? &S.mesh_bound : nullptr);
    V3 albedo = {S.bg, S.bg, S.bg}, n = {0, 0, 0};
    if (best >= 0)
    {
      uint32_t id;
      const bool is_tri = TRIS && (uint32_t)best >= S.n_sph;
      if (!is_tri)
      { /* the winner's normal as trace_step forms it (pt_trace.h: vec3_normalize(point - centre), point_at :257) */
        const V3 p = v_add(o, v_scale(d, min_t));
        const V3 pc = v_sub(p, ld3(S.geom + PT_GEOM_STRIDE * best));
        n = v_scale(pc, rcp_unscaled(sqrt_unscaled(v_dot(pc, pc))));
        id = (uint32_t)best;
      }
      else
      {
        const uint32_t ti = (uint32_t)best - S.n_sph;
        n = ld3(S.tri_normal + 3 * (size_t)ti); /* calculate_surface_normal */
        id = S.tri_object[ti] & ~(PT_HULL_PLUS | PT_HULL_MINUS);
      }
      albedo = ld3(S.color_raw + 3 * (size_t)id);
      const uint32_t flags = (uint32_t)__double_as_longlong(S.mat[PT_MAT_STRIDE * id + 7]);
      if (CHECKER && (flags & PT_FLAG_CHECKER))
      {
        /* restated from trace_step (pt_trace.h, the M_CHECKERED block): hit.u / hit.v as the scan leaves them -- the LAST
         * passing triangle's if the ray passes any (TriLast), else the closest sphere's (:410-411) -- then checkered_texture
         * :386-391 with M = 100000 (:508), here on the colour itself */
        double tex_u, tex_v;
        if (!(TRIS && last.idx >= 0))
        {
          tex_u = atan2_tab(n.x, n.z, S.atan_tab) / (2 * kPi) + 0.5;
          tex_v = n.y * 0.5 + 0.5;
        }
        else
        {
          const double *tx = S.tri_tex + 6 * (size_t)((uint32_t)last.idx - S.n_sph);
          const double lu = last.u, lv = last.v;
          double w0 = 1 - lu - lv;
          tex_u = (tx[0] * w0 + tx[2] * lu) + tx[4] * lv;
          tex_v = (tx[1] * w0 + tx[3] * lu) + tx[5] * lv;
        }
        double on = (double)((frac1(tex_u * 100000.0) > 0.5) ^ (frac1(tex_v * 100000.0) < 0.5));
        double c = 0.3 * (1 - on) + 0.7 * on;
        albedo = v_scale(albedo, c);
      }
      hits++;
      if (min_t < t_min) /* ascending s, strict <: the lowest sample wins a tie */
      {
        t_min = min_t;
        object = id;
      }
    }
    alb_sum = v_add(alb_sum, albedo);
    nrm_sum = v_add(nrm_sum, n);
  }

  const double inv = 1.0 / (double)(uint32_t)L.samples;
  const V3 alb = v_scale(alb_sum, inv), nrm = v_scale(nrm_sum, inv);
  const size_t px3 = (size_t)slot * (PT_TILE_PIXELS * 3) + 3u * lane, px1 = (size_t)slot * PT_TILE_PIXELS + lane;
  if (O.albedo)
  {
    O.albedo[px3 + 0] = inside ? (float)alb.x : 0.f;
    O.albedo[px3 + 1] = inside ? (float)alb.y : 0.f;
    O.albedo[px3 + 2] = inside ? (float)alb.z : 0.f;
  }
  if (O.normal)
  {
    O.normal[px3 + 0] = inside ? (float)nrm.x : 0.f;
    O.normal[px3 + 1] = inside ? (float)nrm.y : 0.f;
    O.normal[px3 + 2] = inside ? (float)nrm.z : 0.f;
  }
  if (O.depth)
    O.depth[px1] = inside ? (float)t_min : 0.f;
  if (O.object)
    O.object[px1] = object;
  if (O.hits)
    O.hits[px1] = hits;
}

/* ---- the AOV kernels (rt_hip_render_aov_tiles): first-hit feature buffers, one list of their own ---------------------------
 * Not members of PT_FAMILY: they trace no path, take no pool, ring, chunk workspace or status word, and no row of the pick table
 * names them.  Which one a launch takes is decided by the scene alone (pt_aov_pick): the forms the scene classes need --
 *   pt_aov_tiles[_chk]          spheres staged, filter staged (sign-test form)
 *   pt_aov_tiles_tri[_chk]      + triangles through the flat filter and the fp32 pre-test
 *   pt_aov_tiles_big[_chk]      spheres staged, filter by scalar loads (more than PT_FILT_LDS_MAX primitives, or a wide range)
 *   pt_aov_tiles_tri_big[_chk]  + triangles through the hierarchy
 *   pt_aov_tiles_mem[_chk]      geometry and materials from memory (pt_geom_in_lds false), triangles (if any) through the hierarchy
 * _chk: the scene has M_CHECKERED materials (u, v tracked).  Body: render_aov<CHECKER, TRIS, FILT_LDS, GEOM_LDS>. */
#define PT_AOV_FAMILY(X) \
  X(A_TILES,           pt_aov_tiles,           render_aov<false, false, true, true>) \
  X(A_TILES_CHK,       pt_aov_tiles_chk,       render_aov<true, false, true, true>) \
  X(A_TRI,             pt_aov_tiles_tri,       render_aov<false, true, true, true>) \
  X(A_TRI_CHK,         pt_aov_tiles_tri_chk,   render_aov<true, true, true, true>) \
  X(A_BIG,             pt_aov_tiles_big,       render_aov<false, false, false, true>) \
  X(A_BIG_CHK,         pt_aov_tiles_big_chk,   render_aov<true, false, false, true>) \
  X(A_TRI_BIG,         pt_aov_tiles_tri_big,   render_aov<false, true, false, true>) \
  X(A_TRI_BIG_CHK,     pt_aov_tiles_tri_big_chk, render_aov<true, true, false, true>) \
  X(A_MEM,             pt_aov_tiles_mem,       render_aov<false, true, false, false>) \
  X(A_MEM_CHK,         pt_aov_tiles_mem_chk,   render_aov<true, true, false, false>)

#define PT_AOV_ENTRY(id, name, ...) \
  extern "C" __global__ __launch_bounds__(PT_BLOCK) void name(const PtLaunch L, const PtAovOut O) { __VA_ARGS__(L, O); }
PT_AOV_FAMILY(PT_AOV_ENTRY)
#undef PT_AOV_ENTRY

enum PtAovKernelId
{
  PT_AOV_FAMILY(PT_LIST_ID) A_COUNT
};
typedef void (*PtAovKernelFn)(const PtLaunch, const PtAovOut);
static PtKernelList<PtEntryInfo<PtAovKernelFn>, A_COUNT> pt_aov_kernels = {{PT_AOV_FAMILY(PT_LIST_INFO)}};

/* ---- a ray of the caller's (the ray-query and the radiance-query kernels): ray i of `rays` as given (a 48-byte record) or
 * get_camera_ray of its (u, v) as start_sample forms it from its two draws; with `normalize` the direction goes through
 * vec3_normalize first.  t_max: the ray's limit, t_max_of[i], or DBL_MAX without such an array (the radiance queries have none).
 * Returns whether the ray is valid: every component finite, | |d|^2 - 1 | <= 2^-13 and the limit not NaN (rt_hip.h); no_rules: in
 * that band but not unit to 2^-40 -- the ray's scan must drop nothing by a conservative rule (query_rays). */
__device__ __forceinline__ bool caller_ray(const PtLaunch &L, const double *rays, const double *t_max_of, uint64_t i, uint32_t camera_uv,
                                           uint32_t normalize, V3 &o, V3 &d, double &t_max_out, bool &no_rules_out)
{
  if (camera_uv)
  { /* get_camera_ray (raytracer.c:375-384), as start_sample forms it from its two draws */
    const double2 uv = reinterpret_cast<const double2 *>(rays)[i];
    const CameraRegs cam = load_camera(L);
    const V3 on_plane = v_add(cam.llc, v_add(v_scale(cam.horizontal, uv.x), v_scale(cam.vertical, uv.y)));
    o = cam.pos;
    d = v_normalize_fast(v_sub(cam.pos, on_plane));
  }
  else
  { /* a 48-byte record: three 16-byte loads */
    const double2 *r = reinterpret_cast<const double2 *>(rays) + 3u * i;
    const double2 a = r[0], b = r[1], c = r[2];
    o = {a.x, a.y, b.x};
    d = {b.y, c.x, c.y};
  }
  if (normalize)
    d = v_normalize_fast(d); /* vec3_normalize (vector.h:53-58): zero gives NaN, an overflowing dot gives zero -- both invalid */
  const double t_max = t_max_of ? t_max_of[i] : L.t_start;
  const double dd = v_dot(d, d);
  const double inf = __longlong_as_double(0x7FF0000000000000ll);
  auto finite = [&](double x) { return __builtin_fabs(x) < inf; }; /* false for NaN */
  const bool valid = finite(o.x) && finite(o.y) && finite(o.z) && finite(d.x) && finite(d.y) && finite(d.z) &&
                     __builtin_fabs(dd - 1.0) <= 0x1p-13 && t_max == t_max;
  const bool no_rules = !(__builtin_fabs(dd - 1.0) <= 0x1p-40);
  t_max_out = t_max;
  no_rules_out = no_rules;
  return valid;
}

/* ---- ray-query body: a lane = one ray of the caller's, a wave = 64 consecutive rays ---------------------------------------------
 * rt_hip.h has the contract.  A lane forms its ray (as given, or get_camera_ray of its (u, v) as start_sample forms it; with
 * `normalize` the direction goes through vec3_normalize first), decides whether it is valid, runs ONE intersect() -- scan_filtered
 * with min_t = DBL_MAX on entry, as render_aov calls it -- and writes the winner's record, or a miss if the winner is not below
 * the ray's t_max.  t_max never enters the scan: no rule sees it, the comparison after the scan is the whole visibility test.
 * The skipping rules of scan_filtered are proven for the renderer's own rays: origins within near_R and directions that are
 * vec3_normalize results.  A ray that starts beyond near_R takes the far_origin route as a bounce from a far wall does.  A ray
 * whose direction is in the contract's band but not unit to rounding (| |d|^2 - 1 | > 2^-40; a vec3_normalize result is within
 * 2^-50) is scanned with no_rules: the bounds at pt_build_filter, tri_may_hit32 and the sign-test form are written for |d| <=
 * 1.0001 and |d|^2 >= 0.9998, which the band satisfies, but their budgets were evaluated at |d| = 1 (the drift of d2 under the
 * pull-back, (1 - |d|^2) (2 tol tca + tol^2), is "1e-14" there and 1e-4 of that product at the band's edge), and a caller's ray
 * is not worth re-deriving them for: the exact tests alone decide it.  The walls are not pruned among themselves (BigPrune is
 * the pooled body's; render_aov does without it too), and the hull-facet rule and the bounding-sphere probe belong to trace_step
 * and the parked walks: no query ray meets them.
 * TRIS / FILT_LDS / GEOM_LDS as render_aov.  No texture is evaluated: no M_CHECKERED twin, no TriLast. */
template <bool TRIS, bool FILT_LDS, bool GEOM_LDS>
__device__ __forceinline__ void query_rays(const PtLaunch &L, const PtQuery &Q)
{
  static_assert(GEOM_LDS || !FILT_LDS, "a staged filter table comes with staged geometry");
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const SceneCtx S = stage_scene<GEOM_LDS, FILT_LDS>(L, lds);
  __syncthreads();

  const uint64_t i = (uint64_t)blockIdx.x * PT_BLOCK + threadIdx.x;
  if (i >= Q.n)
    return; /* the last wave's spare lanes, the last workgroup's spare waves (no barrier follows) */
  V3 o, d;
  double t_max;
  bool no_rules;
  const bool valid = caller_ray(L, Q.rays, Q.t_max, i, Q.camera_uv, Q.normalize, o, d, t_max, no_rules);
  const double inf = __longlong_as_double(0x7FF0000000000000ll);

  double min_t = S.t_start, bary_u = 0, bary_v = 0;
  int best = -1;
  if (valid)
    intersect_scene<TRIS, FILT_LDS, true>(S, o, d, min_t, best, bary_u, bary_v, {.big = false, .no_rules = no_rules});
  const bool hit = valid && best >= 0 && min_t < t_max;
  uint32_t object = 0xFFFFFFFFu, prim = 0xFFFFFFFFu;
  V3 point = {0, 0, 0}, n = {0, 0, 0};
  double bu = 0, bv = 0;
  if (hit)
  {
    point = v_add(o, v_scale(d, min_t)); /* point_at */
    if (!(TRIS && (uint32_t)best >= S.n_sph))
    {
      n = v_normalize_fast(v_sub(point, ld3(S.geom + PT_GEOM_STRIDE * best)));
      object = (uint32_t)best;
    }
    else
    {
      const uint32_t ti = (uint32_t)best - S.n_sph; /* the scan index: upload order, whatever order the hierarchy visited in */
      n = ld3(S.tri_normal + 3 * (size_t)ti);       /* calculate_surface_normal */
      object = S.tri_object[ti] & ~(PT_HULL_PLUS | PT_HULL_MINUS);
      prim = ti;
      /* the reference shows a barycentric only through its texture blend, st0 (1 - u - v) + st1 u + st2 v with the corners (0, 0),
       * (1, 0), (0, 1): 0 w + 1 u + 0 v is u for every u but -0.0 (f < 0 times a zero dot product: a ray through a vertex or along
       * an edge), which the sum with +0 turns into +0.0.  The same sum here. */
      bu = bary_u + 0.0;
      bv = bary_v + 0.0;
    }
  }
  if (Q.status)
    Q.status[i] = valid ? (hit ? 1u : 0u) : 2u;
  if (Q.t)
    Q.t[i] = hit ? min_t : inf;
  if (Q.object)
    Q.object[i] = object;
  if (Q.prim)
    Q.prim[i] = prim;
  if (Q.point)
  {
    double *p = Q.point + 3u * i;
    p[0] = point.x; p[1] = point.y; p[2] = point.z;
  }
  if (Q.normal)
  {
    double *p = Q.normal + 3u * i;
    p[0] = n.x; p[1] = n.y; p[2] = n.z;
  }
  if (Q.bary)
    reinterpret_cast<double2 *>(Q.bary)[i] = double2{bu, bv};
  if (Q.ray)
  {
    double2 *p = reinterpret_cast<double2 *>(Q.ray) + 3u * i;
    p[0] = double2{o.x, o.y}; p[1] = double2{o.z, d.x}; p[2] = double2{d.y, d.z};
  }
}

/* ---- the ray-query kernels (rt_hip_query_rays): a list of their own, like the AOV kernels -- no rows of the pick table.  The
 * scene alone picks the form (pt_query_pick), the five geometric forms of the AOV list:
 *   pt_query_rays          spheres staged, filter staged (sign-test form)
 *   pt_query_rays_tri      + triangles through the flat filter and the fp32 pre-test
 *   pt_query_rays_big      spheres staged, filter by scalar loads
 *   pt_query_rays_tri_big  + triangles through the hierarchy
 *   pt_query_rays_mem      geometry from memory, triangles (if any) through the hierarchy
 * Body: query_rays<TRIS, FILT_LDS, GEOM_LDS>. */
#define PT_QUERY_FAMILY(X) \
  X(Q_RAYS,    pt_query_rays,         query_rays<false, true, true>) \
  X(Q_TRI,     pt_query_rays_tri,     query_rays<true, true, true>) \
  X(Q_BIG,     pt_query_rays_big,     query_rays<false, false, true>) \
  X(Q_TRI_BIG, pt_query_rays_tri_big, query_rays<true, false, true>) \
  X(Q_MEM,     pt_query_rays_mem,     query_rays<true, false, false>)

#define PT_QUERY_ENTRY(id, name, ...) \
  extern "C" __global__ __launch_bounds__(PT_BLOCK) void name(const PtLaunch L, const PtQuery Q) { __VA_ARGS__(L, Q); }
PT_QUERY_FAMILY(PT_QUERY_ENTRY)
#undef PT_QUERY_ENTRY

enum PtQueryKernelId
{
  PT_QUERY_FAMILY(PT_LIST_ID) Q_COUNT
};
typedef void (*PtQueryKernelFn)(const PtLaunch, const PtQuery);
static PtKernelList<PtEntryInfo<PtQueryKernelFn>, Q_COUNT> pt_query_kernels = {{PT_QUERY_FAMILY(PT_LIST_INFO)}};

/* ---- the two front ends of trace_sliced (pt_body_static.h): what an entry of the caller's list is ------------------------------
 * RayFront (rt_hip_trace_rays): entry i is ray i of the caller's, formed and judged by caller_ray as query_rays does and kept in LDS
 * for the lane's later samples; its samples run on the stream (seed, index_first + i, k) with the first two draws -- render()'s
 * jitter -- taken and discarded.  The first scan of a ray in the band that is not unit to 2^-40 runs with no_rules, as query_rays
 * scans it; later bounces are vec3_normalize results (or mirror images of such) and keep the rules. */
struct RayFront
{
  typedef PtTrace Args;
  static constexpr bool RULE_SWITCH = true;
  static constexpr uint32_t RAYS = PT_SLICED_ENTRIES;
  struct Entry
  {
    bool valid, band;
  };
  static __device__ __forceinline__ double *ray_lds() /* [component][ray of the workgroup]: 3 KB, in the ray kernels only */
  {
    __shared__ double ray[6 * RAYS];
    return ray;
  }
  static __device__ __forceinline__ void entry(Entry &E, const PtLaunch &L, const PtTrace &Q, uint64_t i, bool inside, uint32_t slice, uint32_t ray_in_wg)
  {
    double *const ray = ray_lds();
    E.valid = false;
    E.band = false;
    if (inside)
    {
      V3 o, d;
      double no_limit;
      E.valid = caller_ray(L, Q.rays, nullptr, i, Q.camera_uv, Q.normalize, o, d, no_limit, E.band);
      if (slice == 0)
      {
        ray[0 * RAYS + ray_in_wg] = o.x; ray[1 * RAYS + ray_in_wg] = o.y; ray[2 * RAYS + ray_in_wg] = o.z;
        ray[3 * RAYS + ray_in_wg] = d.x; ray[4 * RAYS + ray_in_wg] = d.y; ray[5 * RAYS + ray_in_wg] = d.z;
      }
    }
  }
  static __device__ __forceinline__ uint32_t stream(const PtTrace &Q, const Entry &, uint64_t i) { return Q.index_first + (uint32_t)i; }
  static __device__ __forceinline__ void fresh(Path &P, const PtTrace &, const Entry &, uint64_t pixel_key, uint32_t k, uint32_t ray_in_wg)
  {
    const double *const ray = ray_lds();
    P.rng = sample_state_from_term(pixel_key, sample_term(k));
    (void)rnd(P.rng); /* render()'s two jitter draws (raytracer.c:203-206): a sample of a pixel and a sample of a ray */
    (void)rnd(P.rng); /* with that index see the same draws after them */
    const uint32_t z = opaque_zero() + ray_in_wg; /* (read here, per sample: hoisted, the ray would hold twelve registers for the whole loop) */
    P.o = {ray[0 * RAYS + z], ray[1 * RAYS + z], ray[2 * RAYS + z]};
    P.d = {ray[3 * RAYS + z], ray[4 * RAYS + z], ray[5 * RAYS + z]};
    P.T = {1, 1, 1};
    P.Ls = {0, 0, 0};
    P.depth = 0;
  }
  static __device__ __forceinline__ bool no_rules(const Entry &E, bool first) { return first && E.band; }
  static __device__ __forceinline__ void store_extra(const PtTrace &Q, uint64_t i, uint32_t ray_in_wg)
  {
    const double *const ray = ray_lds();
    if (Q.ray)
    {
      double2 *q = reinterpret_cast<double2 *>(Q.ray) + 3u * i;
      q[0] = double2{ray[0 * RAYS + ray_in_wg], ray[1 * RAYS + ray_in_wg]};
      q[1] = double2{ray[2 * RAYS + ray_in_wg], ray[3 * RAYS + ray_in_wg]};
      q[2] = double2{ray[4 * RAYS + ray_in_wg], ray[5 * RAYS + ray_in_wg]};
    }
  }
};

/* PixelFront (rt_hip_trace_pixels): entry i names pixel p = pixels[i] of the launch's frame (x = p % w, y = p / w); p >= w * h is the
 * invalid entry.  Sample k of the entry is the render's sample sample_first + k of that pixel: the fresh branch is start_sample --
 * the stream (seed, p, s), its first two draws the jitter, get_camera_ray through div_small_int and the unscaled normalize --
 * exactly what render_tiles_static runs per sample; no ray is stored or re-read, so there is no LDS of its own.  The slice of
 * sample k is k mod 4 (the list's own numbering: sample_first shifts the stream, not the reduction).  No first scan runs without
 * the rules: a camera ray is a vec3_normalize result (RULE_SWITCH stays off, as in the render). */
struct PixelFront
{
  typedef PtPixels Args;
  static constexpr bool RULE_SWITCH = false;
  struct Entry
  {
    bool valid;
    uint32_t pixel, px, py;
    CameraRegs cam;
  };
  static __device__ __forceinline__ void entry(Entry &E, const PtLaunch &L, const PtPixels &Q, uint64_t i, bool inside, uint32_t, uint32_t)
  {
    E.pixel = inside ? Q.pixels[i] : 0xFFFFFFFFu;
    E.valid = inside && E.pixel < Q.n_pixels;
    E.px = E.pixel % (uint32_t)L.width;
    E.py = E.pixel / (uint32_t)L.width;
    E.cam = load_camera(L);
  }
  static __device__ __forceinline__ uint32_t stream(const PtPixels &, const Entry &E, uint64_t) { return E.pixel; }
  static __device__ __forceinline__ void fresh(Path &P, const PtPixels &Q, const Entry &E, uint64_t pixel_key, uint32_t k, uint32_t)
  { /* the entry's sample k is the pixel's sample sample_first + k (< 2^31) */
    start_sample(P, E.cam, pixel_key, E.px, E.py, sample_term(Q.sample_first + k));
  }
  static __device__ __forceinline__ bool no_rules(const Entry &, bool) { return false; }
  static __device__ __forceinline__ void store_extra(const PtPixels &, uint64_t, uint32_t) {}
};

/* ---- the ten sliced kernels: the radiance queries (rt_hip_trace_rays) and the pixel refinement (rt_hip_trace_pixels), two lists of
 * their own -- no rows of the pick table -- generated from ONE table, a row per geometric form.  The scene alone picks the row
 * (pt_trace_pick, for both lists, as pt_query_pick); the five forms mirror the static trace_path members K_REFR, K_BIG_REFR,
 * K_TRI_REFR, K_TRI_BIG_REFR and K_MEM, every material's code in each:
 *   pt_trace_{rays,pixels}          spheres staged, filter staged (sign-test form)
 *   pt_trace_{rays,pixels}_big      spheres staged, filter by scalar loads
 *   pt_trace_{rays,pixels}_tri      + triangles through the flat filter and the fp32 pre-test
 *   pt_trace_{rays,pixels}_tri_big  + triangles through the hierarchy
 *   pt_trace_{rays,pixels}_mem      geometry from memory, triangles (if any) through the hierarchy
 * Body: trace_sliced<Front, REFRACT = true, CHECKER = true, TRIS, FILT_LDS, GEOM_LDS>. */
#define PT_SLICED_FAMILY(X) \
  X(T_RAYS,    pt_trace_rays,         pt_trace_pixels,         (PT_BLOCK, PT_MIN_WAVES_REFR),     false, true,  true) \
  X(T_BIG,     pt_trace_rays_big,     pt_trace_pixels_big,     (PT_BLOCK, PT_MIN_WAVES_REFR),     false, false, true) \
  X(T_TRI,     pt_trace_rays_tri,     pt_trace_pixels_tri,     (PT_BLOCK, PT_MIN_WAVES_REFR_TRI), true,  true,  true) \
  X(T_TRI_BIG, pt_trace_rays_tri_big, pt_trace_pixels_tri_big, (PT_BLOCK, PT_MIN_WAVES_REFR_TRI), true,  false, true) \
  X(T_MEM,     pt_trace_rays_mem,     pt_trace_pixels_mem,     (PT_BLOCK),                        true,  false, false)

#define PT_SLICED_ENTRY(id, rays, pixels, bounds, ...) \
  extern "C" __global__ __launch_bounds__ bounds void rays(const PtLaunch L, const PtTrace Q) { trace_sliced<RayFront, true, true, __VA_ARGS__>(L, Q); } \
  extern "C" __global__ __launch_bounds__ bounds void pixels(const PtLaunch L, const PtPixels Q) { trace_sliced<PixelFront, true, true, __VA_ARGS__>(L, Q); }
PT_SLICED_FAMILY(PT_SLICED_ENTRY)
#undef PT_SLICED_ENTRY

enum PtTraceKernelId
{
  PT_SLICED_FAMILY(PT_LIST_ID) T_COUNT
};
typedef void (*PtTraceKernelFn)(const PtLaunch, const PtTrace);
typedef void (*PtPixelKernelFn)(const PtLaunch, const PtPixels);
#define PT_SLICED_RAYS(id, rays, pixels, ...) {#rays, rays},
#define PT_SLICED_PIXELS(id, rays, pixels, ...) {#pixels, pixels},
static PtKernelList<PtEntryInfo<PtTraceKernelFn>, T_COUNT> pt_trace_kernels = {{PT_SLICED_FAMILY(PT_SLICED_RAYS)}};
static PtKernelList<PtEntryInfo<PtPixelKernelFn>, T_COUNT> pt_pixel_kernels = {{PT_SLICED_FAMILY(PT_SLICED_PIXELS)}};
#undef PT_SLICED_RAYS
#undef PT_SLICED_PIXELS

/* The sample count a resolve divides slot `slot` by: the launch's, or -- an accumulation with frozen tiles (rt_hip_accum_freeze) --
 * the slot's own where it has one (0: the slot is live and holds the launch's count). */
__device__ __forceinline__ int32_t resolve_samples(const PtLaunch &L, const uint32_t *tile_samples, uint32_t slot)
{
  const uint32_t own = tile_samples ? tile_samples[slot] : 0u;
  return own ? (int32_t)own : L.samples;
}

/* finish_pixels (pt_trace.h) with the sample count as an argument: the resolve's own copy, statement for statement, so that the
 * members of the family, which finish their one-chunk tiles with finish_pixels, keep the code they had */
__device__ __forceinline__ void resolve_finish_pixels(const PtLaunch &L, int32_t samples, const unsigned long long *sums,
                                                      const unsigned long long *nan_mask, uint32_t tile, float *out_f, uint8_t *out_b)
{
  if (threadIdx.x < PT_TILE_PIXELS * 3)
  {
    const uint32_t t = threadIdx.x / 3u, c = threadIdx.x - 3u * t;
    /* tile_pixel, written out as in finish_pixels: the call moves pt_resolve_tiles */
    const bool inside = (tile % L.tiles_x) * PT_TILE + (t & 7u) < (uint32_t)L.width &&
                        (tile / L.tiles_x) * PT_TILE + (t >> 3) < (uint32_t)L.height;
    const double inv_s = 1.0 / (double)samples;
    double mean = ((double)(long long)sums[threadIdx.x] * L.acc_inv_scale) * inv_s;
    const double quiet_nan = __longlong_as_double(0x7FF8000000000000ll);
    mean = ((nan_mask[c] >> t) & 1ull) ? quiet_nan : mean;
    out_f[threadIdx.x] = inside ? (float)mean : 0.f;
    out_b[threadIdx.x] = inside ? tonemap(mean) : 0;
  }
}

/* Second pass of a chunked render: per-tile fixed-point sums -> float3 + tonemapped bytes.  tile_samples: null, or a count per
 * slot (resolve_samples): the slot is finished exactly as a launch of that many samples finishes it. */
extern "C" __global__ __launch_bounds__(PT_BLOCK) void pt_resolve_tiles(const PtLaunch L, const uint32_t *tile_samples)
{
  __shared__ float out_f[PT_TILE_PIXELS * 3];
  __shared__ uint8_t out_b[PT_TILE_PIXELS * 3 + 64];
  /* (a mixed grid, PtLaunch.n_whole > 0: the grid is the chunked slots, and the workspace holds their records alone) */
  const uint32_t slot = L.n_whole + blockIdx.x;
  const int32_t samples = resolve_samples(L, tile_samples, slot);
  const uint32_t tile = L.tile_first + slot * L.tile_stride;
  if (L.acc_windows)
  { /* the M_REFRACTION forms: windowed sums (win_add), merged chunk by chunk in carry-normalised form */
    if (threadIdx.x < PT_TILE_PIXELS * 3)
    {
      const uint32_t t = threadIdx.x / 3u, c = threadIdx.x - 3u * t;
      /* tile_pixel, written out: the call moves pt_resolve_tiles */
      const bool inside = (tile % L.tiles_x) * PT_TILE + (t & 7u) < (uint32_t)L.width && (tile / L.tiles_x) * PT_TILE + (t >> 3) < (uint32_t)L.height;
      unsigned long long w[PT_WIN_N];
#pragma unroll
      for (int k = 0; k < PT_WIN_N; k++)
        w[k] = L.acc_ws[((size_t)slot * (PT_TILE_PIXELS * 3) + threadIdx.x) * PT_WIN_N + k];
      win_normalize(w);
      double mean = win_value(w) * (1.0 / (double)samples);
      const unsigned long long nan_mask = L.acc_ws[(size_t)L.tile_count * (PT_TILE_PIXELS * 3 * PT_WIN_N) + (size_t)slot * 3 + c];
      mean = ((nan_mask >> t) & 1ull) ? __longlong_as_double(0x7FF8000000000000ll) : mean;
      out_f[threadIdx.x] = inside ? (float)mean : 0.f;
      out_b[threadIdx.x] = inside ? tonemap(mean) : 0;
    }
  }
  else
    resolve_finish_pixels(L, samples, L.acc_ws + (size_t)blockIdx.x * (PT_TILE_PIXELS * 3),
                          L.acc_ws + (size_t)(L.tile_count - L.n_whole) * (PT_TILE_PIXELS * 3) + (size_t)blockIdx.x * 3, tile, out_f, out_b);
  __syncthreads();
  store_tile_pixels(L, out_f, out_b, slot);
}

/* Resolve of an accumulation on the static body (rt_hip_accum_resolve): the slice sums its passes left in L.slice_ws -> pixel
 * means over L.samples (the samples done so far).  Not a member of the family: no scene, no samples.  The lane mapping, the
 * shuffles, the scale and the stores are render_tiles_static's own, so after the whole budget the tile is the one-shot tile bit
 * for bit (the reason is given there). */
extern "C" __global__ __launch_bounds__(PT_BLOCK) void pt_resolve_slices(const PtLaunch L, const uint32_t *tile_samples)
{
  __shared__ float out_f[PT_TILE_PIXELS * 3];
  __shared__ uint8_t out_b[PT_TILE_PIXELS * 3 + 64];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t pix_in_tile = wave * 16u + (lane >> 2);
  const uint32_t slice = lane & (PT_SLICES - 1);
  const uint32_t slot = blockIdx.x;
  const uint32_t tile = L.tile_first + slot * L.tile_stride;
  uint32_t px, py;
  const bool inside = tile_pixel(L.tiles_x, tile, pix_in_tile, L.width, L.height, px, py);
  const double *const sum = L.slice_ws + (size_t)slot * (3u * PT_BLOCK) + threadIdx.x;
  const V3 acc = reduce_slices({sum[0], sum[PT_BLOCK], sum[2 * PT_BLOCK]});
  const V3 mean = v_scale(acc, 1.0 / (double)(uint32_t)resolve_samples(L, tile_samples, slot));
  if (slice == 0)
  {
    out_f[3 * pix_in_tile + 0] = inside ? (float)mean.x : 0.f;
    out_f[3 * pix_in_tile + 1] = inside ? (float)mean.y : 0.f;
    out_f[3 * pix_in_tile + 2] = inside ? (float)mean.z : 0.f;
    out_b[3 * pix_in_tile + 0] = inside ? tonemap(mean.x) : 0;
    out_b[3 * pix_in_tile + 1] = inside ? tonemap(mean.y) : 0;
    out_b[3 * pix_in_tile + 2] = inside ? tonemap(mean.z) : 0;
  }
  __syncthreads();
  store_tile_pixels(L, out_f, out_b, slot);
}

/* ---- adaptive sampling (rt_hip.h: rt_hip_tile_error, rt_hip_accum_freeze) ---------------------------------------------------
 * pt_tile_error: the error estimate of a tile from two resolves of one accumulation, `cur` (means of the first n samples) and
 * `prev` (of the first h < n), compact tile-major.  A wave per tile, a lane per pixel; fp64 in the order rt_hip.h writes, floats
 * widened exactly.  The tile's sum is a butterfly over the lanes: fp64 addition commutes, so lane 0 holds the bits of the tree
 * v[i] += v[i + m], m = 32 .. 1.  No scene, no LDS. */
extern "C" __global__ __launch_bounds__(PT_BLOCK) void pt_tile_error(const float *__restrict__ cur, const float *__restrict__ prev, int width,
                                                                     int height, uint32_t tiles_x, uint32_t tile_first,
                                                                     uint32_t tile_stride, uint32_t tile_count, float *__restrict__ error)
{
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t slot = blockIdx.x * (PT_BLOCK / 64u) + wave;
  if (slot >= tile_count)
    return;
  const uint32_t tile = tile_first + slot * tile_stride;
  const uint32_t tx0 = (tile % tiles_x) * PT_TILE, ty0 = (tile / tiles_x) * PT_TILE;
  const bool inside = tx0 + (lane & 7u) < (uint32_t)width && ty0 + (lane >> 3) < (uint32_t)height; /* tile_pixel, written out: the call moves pt_tile_error */
  const uint32_t valid = min((uint32_t)PT_TILE, (uint32_t)width - tx0) * min((uint32_t)PT_TILE, (uint32_t)height - ty0);
  const size_t at = (size_t)slot * (PT_TILE_PIXELS * 3) + 3u * lane;
  const float c0 = cur[at], c1 = cur[at + 1], c2 = cur[at + 2], p0 = prev[at], p1 = prev[at + 1], p2 = prev[at + 2];
  const bool finite = isfinite(c0) && isfinite(c1) && isfinite(c2) && isfinite(p0) && isfinite(p1) && isfinite(p2);
  double e = 0.0;
  if (inside && finite)
  {
    const double d = (fabs((double)c0 - (double)p0) + fabs((double)c1 - (double)p1)) + fabs((double)c2 - (double)p2);
    double l = ((double)c0 + (double)c1) + (double)c2;
    l = (l > 0.0) ? l : 0.0;
    e = d / sqrt(l + 0x1p-10);
  }
  for (int m = 32; m > 0; m >>= 1)
    e = e + __shfl_xor(e, m);
  if (lane == 0)
    error[slot] = (float)(e / (double)valid);
}

/* pt_tile_keep: keep[k] = 1 iff slot k is live (tile_samples[k] == 0) and some slot u of the launch whose tile lies within
 * Chebyshev distance `dilate` of slot k's tile, in the image's tile grid, has !(error[u] <= threshold); tiles that are not in
 * the launch (tile_stride > 1) do not vote.  A thread per slot. */
extern "C" __global__ __launch_bounds__(256) void pt_tile_keep(const float *__restrict__ error, const uint32_t *__restrict__ tile_samples,
                                                               uint32_t tiles_x, uint32_t tiles_y, uint32_t tile_first, uint32_t tile_stride,
                                                               uint32_t tile_count, double threshold, int dilate, uint8_t *__restrict__ keep)
{
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  if (k >= tile_count)
    return;
  const uint32_t tile = tile_first + k * tile_stride;
  const int tx = (int)(tile % tiles_x), ty = (int)(tile / tiles_x);
  bool vote = false;
  for (int dy = -dilate; dy <= dilate; dy++)
    for (int dx = -dilate; dx <= dilate; dx++)
    {
      const int x = tx + dx, y = ty + dy;
      if (x < 0 || y < 0 || x >= (int)tiles_x || y >= (int)tiles_y)
        continue;
      const uint32_t t = (uint32_t)y * tiles_x + (uint32_t)x;
      if (t < tile_first)
        continue;
      const uint32_t off = t - tile_first;
      const uint32_t u = tile_stride ? off / tile_stride : 0u;
      if (u >= tile_count || u * tile_stride != off)
        continue;
      vote = vote || !((double)error[u] <= threshold);
    }
  keep[k] = (vote && tile_samples[k] == 0u) ? 1 : 0;
}

/* pt_tile_compact: the freeze itself.  A live slot (tile_samples[k] == 0) that keep[k] does not keep is frozen at `done` samples;
 * the slots still live go to slot_list in ascending order -- the list is a function of the mask alone -- and their number to
 * *live_count.  One workgroup: thread i owns the slots [i * per, (i + 1) * per), counts, scans the counts, then writes. */
#define PT_COMPACT_THREADS 1024
extern "C" __global__ __launch_bounds__(PT_COMPACT_THREADS) void pt_tile_compact(const uint8_t *__restrict__ keep, uint32_t *__restrict__ tile_samples,
                                                                               uint32_t tile_count, uint32_t done, uint32_t *__restrict__ slot_list,
                                                                               uint32_t *__restrict__ live_count)
{
  __shared__ uint32_t part[PT_COMPACT_THREADS];
  const uint32_t per = (tile_count + PT_COMPACT_THREADS - 1u) / PT_COMPACT_THREADS;
  const uint32_t k0 = min(tile_count, threadIdx.x * per), k1 = min(tile_count, k0 + per);
  uint32_t n = 0;
  for (uint32_t k = k0; k < k1; k++)
  {
    const bool live = tile_samples[k] == 0u;
    if (live && !keep[k])
      tile_samples[k] = done;
    n += (live && keep[k]) ? 1u : 0u;
  }
  part[threadIdx.x] = n;
  __syncthreads();
  for (uint32_t step = 1; step < PT_COMPACT_THREADS; step <<= 1)
  { /* inclusive scan (Hillis-Steele) */
    const uint32_t add = threadIdx.x >= step ? part[threadIdx.x - step] : 0u;
    __syncthreads();
    part[threadIdx.x] += add;
    __syncthreads();
  }
  uint32_t at = part[threadIdx.x] - n;
  for (uint32_t k = k0; k < k1; k++)
    if (tile_samples[k] == 0u)
      slot_list[at++] = k;
  if (threadIdx.x == PT_COMPACT_THREADS - 1)
    *live_count = part[threadIdx.x];
}

/* Self-test hook (rt_hip_selftest_math): evaluates the kernel's exact-arithmetic shortcuts
 * on caller data so a test can compare them bit for bit with the host's IEEE results.
 * op 0: sqrt_unscaled(a[i]);  op 1: div_small_int(a[i], b[i], 1/b[i]);  op 2: the library
 * sqrt(a[i]);  op 3: a[i] / b[i];  op 4: rnd_pm1-style fused r * 2^-30 - 1 with r = a[i];  op 5: rcp_unscaled(a[i]);
 * op 6: atan2_tab(a[i], b[i]);  op 7: frac1(a[i]) (= fmod(a[i], 1.0));  op 8: win_add of every a[i] into one accumulator (out[0..6]);
 * op 9: win_normalize, then win_value, of the PT_WIN_N words a[8 g .. 8 g + 6) (bit patterns) -> out[8 g ..]: the words, the value. */
extern "C" __global__ __launch_bounds__(256) void pt_selftest_math(int op, const double *a, const double *b,
                                                                  double *out, size_t n)
{
  __shared__ double tab[PT_ATAN_TAB];
  atan_table_to_lds(tab);
  __syncthreads();
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
  {
    double r = 0;
    if (op == 0)
      r = sqrt_unscaled(a[i]);
    else if (op == 1)
      r = div_small_int(a[i], b[i], 1.0 / b[i]);
    else if (op == 2)
      r = sqrt(a[i]);
    else if (op == 3)
      r = a[i] / b[i];
    else if (op == 4)
      r = __builtin_fma(a[i], 1.0 / 1073741824.0, -1.0);
    else if (op == 5)
      r = rcp_unscaled(a[i]);
    else if (op == 6)
      r = atan2_tab(a[i], b[i], tab);
    else if (op == 7)
      r = frac1(a[i]);
    else if (op == 8)
    { /* the windowed pixel sums of pt_render_tiles_refr_pool: every a[i] into ONE accumulator, out[0 .. PT_WIN_N) (as the caller
       * initialised it: zeros, or words that start near the capacity); out[PT_WIN_N] counts the values win_add refused
       * (non-finite, or at least 2^128) */
      if (!win_add(reinterpret_cast<unsigned long long *>(out), a[i]))
        atomicAdd(reinterpret_cast<unsigned long long *>(out) + PT_WIN_N, 1ull);
      continue;
    }
    else if (op == 9)
    { /* how a chunk's window is merged and read (pt_resolve_tiles): one group of eight doubles per lane */
      if ((i & 7u) == 0u && i + 8u <= n)
      {
        unsigned long long w[PT_WIN_N];
        for (int k = 0; k < PT_WIN_N; k++)
          w[k] = (unsigned long long)__double_as_longlong(a[i + k]);
        win_normalize(w);
        for (int k = 0; k < PT_WIN_N; k++)
          out[i + k] = __longlong_as_double((long long)w[k]);
        out[i + PT_WIN_N] = win_value(w);
        out[i + PT_WIN_N + 1] = 0.0;
      }
      continue;
    }
    out[i] = r;
  }
}

/* Self-test hook (rt_hip_selftest_intersect): the kernel's own exact primitive tests and its
 * phase-1 filter on caller data, one lane per case, so that known-answer vectors generated by
 * the compiled reference (tests/golden/primitives.npz) reach exact_sphere / exact_triangle /
 * filter_chunk themselves and not only their host twins.
 *   kind 0: prims = n x 4 (cx cy cz r*r), the record exact_sphere reads in the render kernels;
 *   kind 1: prims = n x 9 (v0, e1, e2), the record exact_triangle reads.
 * Case i = ray i against primitive i: hit[i], tuv[3i..] = t, and for triangles the barycentric
 * u, v the render kernels blend texture coordinates with.
 * Filter: one workgroup (one wavefront) per block of 64 cases; `filt` is the table
 * pt_build_filter made of all n primitives for near_R, so block b's pairs are those of the 64
 * primitives of the block.  Every lane runs phase 1 over them with its own ray, in the three
 * forms the render kernels use, and stores the 64-bit keep masks:
 *   keep[3i + 0]  spheres: sign-test form from LDS (pt_render_tiles); triangles: the per-lane fp32
 *                 Moeller-Trumbore pre-test (tri_may_hit32) instead
 *   keep[3i + 1]  compare form from LDS, push_keep_bit (pt_render_tiles_tri)
 *   keep[3i + 2]  compare form, table by scalar loads (the _big kernels)
 * bit j = ray i keeps primitive 64 b + j.  A test can so check 64 n (ray, primitive) pairs:
 * the filter must keep every pair the exact test accepts. */
extern "C" __global__ __launch_bounds__(64) void pt_selftest_intersect(int kind, const double *rays, const double *prims,
                                                                      const f32x2 *filt, const float4 *tri32, uint32_t n,
                                                                      double near_R2, double filt_shift, double t_start,
                                                                      uint8_t *hit, double *tuv, unsigned long long *keep)
{
  __shared__ f32x2 filt_lds[PT_FILT_STRIDE * 33]; /* 32 pairs + the look-ahead pair */
  const uint32_t base = blockIdx.x * 64u;
  const uint32_t chunk = min(64u, n - base);
  for (uint32_t k = threadIdx.x; k < PT_FILT_STRIDE * 33; k += 64)
    filt_lds[k] = filt[PT_FILT_STRIDE * (size_t)(base >> 1) + k];
  __syncthreads();
  const uint32_t i = base + threadIdx.x;
  const bool live = i < n;
  const uint32_t src = live ? i : base; /* idle lanes of the last block shadow its first case */
  const V3 o = ld3(rays + 6 * (size_t)src), d = ld3(rays + 6 * (size_t)src + 3);

  double min_t = t_start, bu = 0, bv = 0;
  int best = -1;
  if (kind == 0)
    exact_sphere(prims + 4 * (size_t)src, 0u, o, d, min_t, best);
  else
    exact_triangle(prims + 9 * (size_t)src, 0u, o, d, min_t, best, bu, bv);

  uint32_t lo, hi;
  unsigned long long m0 = ~0ull, m1, m2;
  if (kind == 0)
  {
    const FiltRay fs = filter_ray<true>(o, d, filt_shift, near_R2);
    filter_chunk<false, true>(filt_lds, 0u, chunk, fs, lo, hi);
    m0 = ((unsigned long long)hi << 32) | lo;
  }
  const FiltRay fr = filter_ray<false>(o, d, filt_shift, near_R2);
  if (kind == 1)
  { /* the per-lane fp32 pre-test (tri_may_hit32) of this ray against every triangle of the block */
    m0 = 0;
    for (uint32_t j = 0; j < chunk; j++)
      if (fr.far_origin || tri_may_hit32(tri32 + (PT_TRI32_STRIDE / 4) * (size_t)(base + j), fr.ox, fr.oy, fr.oz, fr.dx.x, fr.dy.x, fr.dz.x))
        m0 |= 1ull << j;
  }
  filter_chunk<true, true>(filt_lds, 0u, chunk, fr, lo, hi);
  m1 = ((unsigned long long)hi << 32) | lo;
  filter_chunk<false, false>(filt, base, chunk, fr, lo, hi);
  m2 = ((unsigned long long)hi << 32) | lo;
  if (live)
  {
    hit[i] = best >= 0 ? 1 : 0;
    tuv[3 * (size_t)i + 0] = min_t;
    tuv[3 * (size_t)i + 1] = bu;
    tuv[3 * (size_t)i + 2] = bv;
    keep[3 * (size_t)i + 0] = m0;
    keep[3 * (size_t)i + 1] = m1;
    keep[3 * (size_t)i + 2] = m2;
  }
}

/* Self-test hook (rt_hip_selftest_intersect, kind 2): the keep words of phase 1 on the fp16 matrix pipe (filter_mfma16), on
 * caller data.  prims = n x 4 (cx cy cz r*r) as for kind 0, n a multiple of 64.  One wavefront per block of 64 rays and 64
 * spheres; the block's first 32 spheres are the matrix rows (pt_mfma16_row, built here as the pooled body's prologue builds
 * them, first = 0), its other 32 go through the packed loop behind them, as in a scene of more than 32 small spheres.
 * Every lane runs its own ray against the block's 64 spheres:
 *   keep[3i + 0]  packed sign-test form alone (what -DPT_MFMA16=0 computes)
 *   keep[3i + 1]  matrix pipe for spheres 0..31, merged by filter_chunk as in the render kernels
 *   keep[3i + 2]  the kernel's exact test (exact_sphere), bit j = ray i hits sphere 64 b + j
 * hit[i] = 1 when all 32 rows fit the form (else the block ran the packed loop twice); tuv[3i], tuv[3i + 1] = the matrix pipe's
 * tca16 and ll16 of ray 64 b + (i % 32) and sphere 64 b + 16 ((i % 64) / 32): values a test can set against fp64 and the bounds ET, EL
 * of pt_mfma16_row. */
extern "C" __global__ __launch_bounds__(64) void pt_selftest_mfma16(const double *rays, const double *prims, const double *entry_src,
                                                                   const f32x2 *filt, uint32_t n, double near_R, double near_R2,
                                                                   double filt_shift, uint8_t *hit, double *tuv, unsigned long long *keep)
{
  __shared__ f32x2 filt_lds[PT_FILT_STRIDE * 33];
  __shared__ u32x4_t mf_a[64];
  __shared__ uint32_t mf_bad;
  const uint32_t base = blockIdx.x * 64u; /* base + 64 <= n */
  if (threadIdx.x == 0)
    mf_bad = 0u;
  for (uint32_t k = threadIdx.x; k < PT_FILT_STRIDE * 33; k += 64)
    filt_lds[k] = filt[PT_FILT_STRIDE * (size_t)(base >> 1) + k];
  __syncthreads();
  if (threadIdx.x < PT_MFMA16_ROWS)
  {
    uint16_t row[16];
    if (!pt_mfma16_row(entry_src + PT_ENTRY_SRC_STRIDE * (size_t)(base + threadIdx.x), near_R, filt_shift, row))
      atomicOr(&mf_bad, 1u);
    const uint32_t m = mfma16_row_of(threadIdx.x);
#pragma unroll
    for (int h = 0; h < 2; h++)
      mf_a[32 * h + m] = u32x4_t{row[8 * h + 0] | ((uint32_t)row[8 * h + 1] << 16), row[8 * h + 2] | ((uint32_t)row[8 * h + 3] << 16),
                                 row[8 * h + 4] | ((uint32_t)row[8 * h + 5] << 16), row[8 * h + 6] | ((uint32_t)row[8 * h + 7] << 16)};
  }
  __syncthreads();
  const Mfma16 MF = {mf_a, 0u, __builtin_amdgcn_readfirstlane((int)mf_bad) == 0};
  const uint32_t i = base + threadIdx.x;
  const V3 o = ld3(rays + 6 * (size_t)i), d = ld3(rays + 6 * (size_t)i + 3);
  const FiltRay fr = filter_ray<true, true>(o, d, filt_shift, near_R2);
  uint32_t lo, hi;
  filter_chunk<false, true>(filt_lds, 0u, 64u, fr, lo, hi);
  const unsigned long long m0 = ((unsigned long long)hi << 32) | lo;
  PreCand pre = {0u, 0u, false};
  float probe[2] = {0.f, 0.f};
  if (MF.on)
  {
    pre.drop = filter_mfma16<true>(MF, fr, probe);
    pre.on = true;
  }
  filter_chunk<false, true>(filt_lds, 0u, 64u, fr, lo, hi, BigPrune{nullptr, 0u}, nullptr, pre);
  const unsigned long long m1 = ((unsigned long long)hi << 32) | lo;
  unsigned long long m2 = 0ull;
  for (uint32_t j = 0; j < 64u; j++)
  {
    double t = 1.7976931348623157e308;
    int best = -1;
    exact_sphere(prims + 4 * (size_t)(base + j), 0u, o, d, t, best);
    m2 |= best >= 0 ? (1ull << j) : 0ull;
  }
  hit[i] = MF.on ? 1 : 0;
  tuv[3 * (size_t)i + 0] = (double)probe[0];
  tuv[3 * (size_t)i + 1] = (double)probe[1];
  tuv[3 * (size_t)i + 2] = 0.0;
  keep[3 * (size_t)i + 0] = m0; /* (filter_chunk has given far-origin lanes every bit) */
  keep[3 * (size_t)i + 1] = m1;
  keep[3 * (size_t)i + 2] = m2;
}

/* Self-test hook (rt_hip_selftest_xcc): which XCD each workgroup of a launch ran on, as the parked-walk kernels read it
 * (pt_park_acquire): counts[x] = workgroups that saw HW_REG_XCC_ID == x. */
extern "C" __global__ __launch_bounds__(64) void pt_selftest_xcc(unsigned int *counts)
{
  if (threadIdx.x == 0)
    atomicAdd(&counts[(uint32_t)__builtin_amdgcn_s_getreg(20 | (0 << 6) | (3 << 11)) & 15u], 1u);
}

hipError_t pt_launch_selftest_xcc(unsigned int *counts, uint32_t n_workgroups, hipStream_t stream)
{
  hipLaunchKernelGGL(pt_selftest_xcc, dim3(n_workgroups), dim3(64), 0, stream, counts);
  return hipGetLastError();
}

hipError_t pt_launch_selftest(int op, const double *a, const double *b, double *out, size_t n, hipStream_t stream)
{
  hipLaunchKernelGGL(pt_selftest_math, dim3(256), dim3(256), 0, stream, op, a, b, out, n);
  return hipGetLastError();
}

/* Builds the packed-fp32 phase-1 filter table for one launch (the thresholds depend on
 * near_R, i.e. on the camera).  Per pair: cx cy cz r2_hi neg_tol, two primitives per f32x2.
 * Bound (e = 2^-24, fp32 unit roundoff; a = |c| + |o| <= A := |c| + near_R; |d| <= 1.0001):
 *   c, o, d are rounded to fp32 (relative e each), L = c - o adds one rounding, so
 *   |L32 - L| <= 2.01 e a per component; each 3-term fused dot product adds <= 3 e of its
 *   magnitude.  Hence  |tca32 - tca| <= 6.2 e A   and   |d2_32 - d2| <= 20.5 e A^2,  where tca,
 *   d2 are the real-number values; the reference's own fp64 rounding of them (~1e-16
 *   relative) is absorbed by the 1.5x slack:
 *     drop  <=>  tca32 < -(Rb + 10 e A)   or   d2_32 > R2 + 32 e A^2       (never a false drop)
 *   sphere: R2 = r*r, Rb = 0 (intersect_sphere rejects tca < 0, raytracer.c:84);
 *   triangle: R2 = Rb^2 of its bounding sphere, Rb = that radius (the hit point is inside the
 *   bounding sphere, so the centre is at most Rb behind the origin).
 * Thresholds are rounded away from the accept region when stored as fp32. */
/* fp32 hierarchy nodes for one launch: the planes of a node's two children as (child 0,
 * child 1) pairs, boxes widened by 4 e (near_R + |b|) and rounded outward (see bvh_traverse);
 * then the two child references. */
extern "C" __global__ __launch_bounds__(256) void pt_build_bvh(const double *bvh_src, uint32_t n_nodes, double near_R,
                                                              float *nodes)
{
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_nodes; i += gridDim.x * blockDim.x)
  {
    const double *src = bvh_src + PT_BVH_SRC_DOUBLES * (size_t)i;
    float *dst = nodes + PT_BVH_NODE_WORDS * (size_t)i;
    const double e = 5.9604644775390625e-08;
    for (int c = 0; c < 2; c++)
      for (int k = 0; k < 3; k++)
      {
        const double lo = src[6 * c + k], hi = src[6 * c + 3 + k];
        dst[4 * k + c] = __double2float_rd(lo - 4.0 * e * (near_R + fabs(lo)));
        dst[4 * k + 2 + c] = __double2float_ru(hi + 4.0 * e * (near_R + fabs(hi)));
      }
    const uint32_t *refs = reinterpret_cast<const uint32_t *>(src + 12);
    dst[12] = __uint_as_float(refs[0]);
    dst[13] = __uint_as_float(refs[1]);
    dst[14] = 0.f;
    dst[15] = 0.f;
  }
}

/* HULL FACETS (scene creation, once): triangle F is one if every corner p of every triangle of the scene has
 * m . (p - v0_F) <= tau for m = +n_F (PT_HULL_PLUS: the stored normal points outward) or m = -n_F (PT_HULL_MINUS).
 * What it buys (render_tiles_queued): a ray that starts at a hit point on F -- within delta of F's plane -- with
 * m . d > mu has m . (o + t d - v0) >= t mu - delta, so it can meet a triangle point only at t <= (tau + delta) / mu;
 * the launch picks mu so that this is below EPSILON / 4 (rt_hip_shim.hip, hull_margin_for), where intersect_triangle
 * rejects the hit (t > EPSILON, raytracer.c:150): the ray cannot hit any triangle, whatever the mesh looks like
 * elsewhere.  Every facet of a convex mesh is one; of config 5's bounces off the mesh 42 % of all hierarchy walks
 * were such rays, each ~15 node visits to find nothing (PT_DIAG counters, profiles/).  One thread per triangle over
 * all 3 n corners: quadratic, so only up to PT_HULL_MAX_TRIS triangles (3 x 10^8 plane tests for config 5: ~1 ms). */
extern "C" __global__ __launch_bounds__(256) void pt_build_hull_flags(const double *__restrict__ tri_geom,
                                                                      const double *__restrict__ tri_normal, uint32_t n_tri,
                                                                      double tau, uint32_t *tri_object)
{
  __shared__ double corner[3 * 256][3];
  const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = f < n_tri;
  const double *g = tri_geom + 9 * (size_t)(live ? f : 0u);
  const double *nn = tri_normal + 3 * (size_t)(live ? f : 0u);
  const double nx = nn[0], ny = nn[1], nz = nn[2], vx = g[0], vy = g[1], vz = g[2];
  double smax = -1.7976931348623157e308, smin = 1.7976931348623157e308;
  bool bad = !(nx == nx) || !(ny == ny) || !(nz == nz); /* a degenerate triangle has no plane */
  {
    /* shape: the bound on how far a computed hit point lies from F's plane grows with |e1||e2| / |e1 x e2| (the
     * rounding of intersect_triangle's t; derivation at hull_margin_for): facets sharper than 1/16 go without a flag */
    const double cx = g[4] * g[8] - g[5] * g[7], cy = g[5] * g[6] - g[3] * g[8], cz = g[3] * g[7] - g[4] * g[6];
    const double e1 = g[3] * g[3] + g[4] * g[4] + g[5] * g[5], e2 = g[6] * g[6] + g[7] * g[7] + g[8] * g[8];
    bad |= !((cx * cx + cy * cy + cz * cz) * 256.0 >= e1 * e2) || !(e1 * e2 > 0.0);
  }
  for (uint32_t base = 0; base < n_tri; base += 256)
  {
    __syncthreads();
    const uint32_t t = base + threadIdx.x;
    if (t < n_tri)
    {
      const double *q = tri_geom + 9 * (size_t)t;
      for (int k = 0; k < 3; k++)
        for (int a = 0; a < 3; a++)
          corner[3 * threadIdx.x + k][a] = k == 0 ? q[a] : q[a] + q[3 * k + a]; /* v0, v0 + e1, v0 + e2: as the kernels see it */
    }
    __syncthreads();
    const uint32_t n = 3u * min(256u, n_tri - base);
    for (uint32_t c = 0; c < n; c++)
    {
      const double s = (nx * (corner[c][0] - vx) + ny * (corner[c][1] - vy)) + nz * (corner[c][2] - vz);
      smax = fmax(smax, s);
      smin = fmin(smin, s);
      bad |= !(s == s);
    }
  }
  if (live)
  {
    uint32_t bits = 0u;
    if (!bad && smax <= tau)
      bits = PT_HULL_PLUS;
    else if (!bad && smin >= -tau)
      bits = PT_HULL_MINUS;
    tri_object[f] = (tri_object[f] & ~(PT_HULL_PLUS | PT_HULL_MINUS)) | bits;
  }
}

/* The fp32 triangle table of tri_may_hit32 for one near_R: v0, e1, e2 rounded to nearest, the four
 * thresholds formed in fp64 and rounded up. */
extern "C" __global__ __launch_bounds__(256) void pt_build_tri32(const double *tri_geom, uint32_t n_tri, double near_R,
                                                                float *out)
{
  for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < n_tri; t += gridDim.x * blockDim.x)
  {
    const double *g = tri_geom + 9 * (size_t)t;
    float *f = out + PT_TRI32_STRIDE * (size_t)t;
    for (int k = 0; k < 9; k++)
      f[k] = (float)g[k];
    const double e = 5.9604644775390625e-08;
    const double l0 = sqrt(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]), l1 = sqrt(g[3] * g[3] + g[4] * g[4] + g[5] * g[5]),
                 l2 = sqrt(g[6] * g[6] + g[7] * g[7] + g[8] * g[8]);
    const double S = (near_R + l0) * 1.0001;
    const double up = 1.0 + 4.0 * e;
    double Ea = 16.0 * e * l1 * l2 * up, KU = 20.0 * e * S * l2 * up, KV = 20.0 * e * S * l1 * up, KT = 20.0 * e * S * l1 * l2 * up;
    /* products near fp32's range (or non-finite input): the pre-test keeps the triangle whatever it computes */
    if (!(S * l1 * l2 < 1e30) || !(l1 * l2 < 1e30))
      Ea = __longlong_as_double(0x7FF0000000000000ll);
    f[9] = __double2float_ru(Ea);
    f[10] = __double2float_ru(KU);
    f[11] = __double2float_ru(KV);
    f[12] = __double2float_ru(KT);
    f[13] = f[14] = f[15] = 0.f;
  }
}

extern "C" __global__ __launch_bounds__(256) void pt_build_filter(const double *entry_src, uint32_t n_entries,
                                                                 double near_R, float *filt)
{
  const uint32_t n_slots = (n_entries + 1u) & ~1u;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_slots; i += gridDim.x * blockDim.x)
  {
    float *f = filt + 2 * PT_FILT_STRIDE * (size_t)(i >> 1) + (i & 1u);
    if (i < n_entries)
    {
      const double *src = entry_src + PT_ENTRY_SRC_STRIDE * (size_t)i; /* cx cy cz R2 |c| Rb */
      const double e = 5.9604644775390625e-08;                          /* 2^-24 */
      const double A = src[4] + near_R;
      f[0] = (float)src[0];
      f[2] = (float)src[1];
      f[4] = (float)src[2];
      /* (1 + 8 e): one e for this conversion, the rest for the roundings of the chain that
       * carries -r2_hi as its addend (scan_filtered, SHIFT form: 3 e max(r2_hi, A^2)) */
      f[6] = (float)((src[3] + 32.0 * e * A * A) * (1.0 + 8.0 * e));
      f[8] = -(float)((src[5] + 10.0 * e * A) * (1.0 + 4.0 * e));
      /* sign-test form (spheres, small scenes): kq = |c|^2 - r2_hi', formed in fp64 and rounded DOWN, with its
       * own widening r2_hi' = R2 + 40 e A^2 + 8 e | |c|^2 - R2 | (pt_sign_widen_r2).  Bound behind it (e = 2^-24, every input
       * rounded to fp32, fused 3-term chains, o' the pulled-back origin, |o'| <= near_R + tol_max; the bound is stated with
       * A' = |c| + near_R + tol_max while the code forms A = |c| + near_R: tol_max = 12 e (max |c| + near_R) <= 7.2e-7 A, so
       * A'^2 <= (1 + 1.5e-6) A^2 -- inside the 40 over 28 slack of the widening by five orders of magnitude):
       *   tca32 = fma(cz,dz, fma(cy,dy, fma(cx,dx, -o'.d))):  |tca32 - tca'| <= 8.2 e A   (2 e |c| inputs, 3 e A chain,
       *           5.1 e |o'| for o'.d);
       *   ll32  = fma(cz,-2oz, fma(cy,-2oy, fma(cx,-2ox, kq + |o'|^2))):
       *           |ll32 - (|c-o'|^2 - r2_hi')| <= e (5 |kq| + 9.1 |o'|^2 + 10 |c||o'|) <= 10 e A^2 + 5 e |kq|;
       *   q32   = fma(tca32, tca32, -ll32):  |q32 - (r2_hi' - d2)| <= 2 A 8.2 e A + e A^2 + 10 e A^2 + 5 e |kq|
       *           <= 28 e A^2 + 5 e |kq|  <  the widening (|kq| <= | |c|^2 - R2 | + 40 e A^2),
       * so d2 <= R2 in exact arithmetic implies q32 >= 0: never a false drop (the PT_DIAG build re-checks every
       * dropped sphere with the exact test: 0 violations). */
      {
        const double cc = src[4] * src[4]; /* |c| was rounded up by 1e-12: inside the slack */
        const double g = fabs(cc - src[3]);
        /* pt_device.h: the widening shared with the host's big_prune_for (= (40 e A^2 + 8 e g)(1 + 8 e), then 4 e g) */
        f[10] = __double2float_rd((cc - (src[3] + pt_sign_widen_r2(A, g))) - pt_sign_widen_kq(g));
      }
    }
    else
    { /* padding slot of an odd count: masked out by valid_lo / valid_hi in the scan */
      f[0] = f[2] = f[4] = 0.f;
      f[6] = -1.f;
      f[8] = 0.f;
      f[10] = 0.f;
    }
  }
}

/* ---- launch wrappers (host side), declared in pt_device.h ---------------------- */

size_t pt_render_lds_bytes(const PtSceneView &sc)
{
  if (!pt_geom_in_lds(sc))
    return 0;
  size_t doubles = PT_GEOM_STRIDE * (size_t)sc.n_spheres + PT_MAT_STRIDE * (size_t)(sc.n_spheres + sc.n_meshes);
  const size_t n_entries = (size_t)sc.n_spheres + sc.n_triangles;
  if (pt_filter_in_lds(sc))
    doubles += pt_filt_pair_slots((uint32_t)n_entries) + (size_t)sc.n_triangles * (PT_TRI32_STRIDE / 2); /* f32x2 = one double-sized slot */
  return doubles * sizeof(double);
}

/* ---- which member a launch takes: ONE table ------------------------------------------------------------------------------
 * A launch is classified by the six things the family is split by, and the first row of pt_pick_table that matches names the
 * kernel.  The fallbacks (no ring workspace, windowed sums that do not fit, a pending-ray pool that could not be had at
 * 4 x 512 stacks, scenes beyond fp32's comfortable range) are rows like any other.  A row field of ANY matches everything.
 *
 *   integ   PATH trace_path (raytracer.c:482-554) | CAST cast_ray (:556-641)
 *   stage   STAGED   sphere geometry + materials fit the LDS staging budget and are staged
 *           STREAM   they would fit, but the scene is a sphere scene of more than ~85 spheres: faster streamed (pt_stream_sized)
 *           LARGE    beyond the staging budget (pt_geom_in_lds false)
 *   mesh    NONE | FLAT triangles scanned through the flat filter staged in LDS (pt_filter_in_lds) | HIER triangles through the
 *           hierarchy | HIERBIG the same with more than PT_FILT_LDS_MAX triangles (what a scene beyond the staging budget needs
 *           for parked walks: HIERBIG rows also match where HIER is asked for -- see pt_row_matches)
 *   mat     PLAIN | CHK any M_CHECKERED | REFR any M_REFRACTION (wins over CHK: the _refr bodies carry the checker code) |
 *           for CAST: GLASS2 a material with M_REFLECTION and M_REFRACTION (two children per hit), else PLAIN
 *   range   NORMAL | WIDE a centre or radius beyond 1e17 (NaN-safe compare filter, no sign tests, no parked walks)
 *   park    YES the parked-walk body may run: its workspace exists and references fit 24-bit stack entries | NO
 *   round   YES the mesh's bounding sphere shows a ray no more than its box (probe = the sphere alone) | NO
 *   fit     YES the windowed sums of the pooled refraction kernels hold this launch (pt_refr_pool_fits per chunk) and, for the
 *           parked-walk refraction kernels, the pending-ray pool has 4 x 512 stacks per slot | NO
 */
enum { ANY = -1 };
enum PtInteg { PATH = 0, CAST = 1 };
enum PtStage { STAGED = 0, STREAM = 1, LARGE = 2 };
enum PtMesh { NONE = 0, FLAT = 1, HIER = 2, HIERBIG = 3 };
enum PtMat { PLAIN = 0, CHK = 1, REFR = 2, GLASS2 = 3 };
enum PtYesNo { NO = 0, YES = 1 };
enum PtRange { NORMAL = 0, WIDE = 1 };
struct PtPickKey
{
  int integ, stage, mesh, mat, range, park, round, fit;
};
struct PtPickRow
{
  int integ, stage, mesh, mat, range, park, round, fit;
  int kernel;
};
static const PtPickRow pt_pick_table[] = {
    /* integ stage   mesh     mat     range   park round fit   kernel */
    /* ---- cast_ray: the static body; two-child materials or a scene beyond the staging budget: the general in-memory kernel */
    {CAST, LARGE,  ANY,     ANY,    ANY,    ANY, ANY, ANY, K_WHITTED_MEM},
    {CAST, ANY,    ANY,     GLASS2, ANY,    ANY, ANY, ANY, K_WHITTED_MEM},
    {CAST, ANY,    NONE,    ANY,    NORMAL, ANY, ANY, ANY, K_WHITTED},
    {CAST, ANY,    NONE,    ANY,    WIDE,   ANY, ANY, ANY, K_WHITTED_BIG},
    {CAST, ANY,    FLAT,    ANY,    ANY,    ANY, ANY, ANY, K_WHITTED_TRI},
    {CAST, ANY,    HIER,    ANY,    ANY,    ANY, ANY, ANY, K_WHITTED_TRI_BIG},
    /* ---- trace_path, scenes beyond the staging budget */
    {PATH, LARGE,  NONE,    REFR,   NORMAL, ANY, ANY, YES, K_REFR_POOL_MEM},
    {PATH, LARGE,  ANY,     REFR,   ANY,    ANY, ANY, ANY, K_MEM},              /* ... with a mesh, out of range, or sums that do not fit: the static body */
    {PATH, LARGE,  HIERBIG, PLAIN,  NORMAL, YES, ANY, ANY, K_TRI_QUEUED_MEM},
    {PATH, LARGE,  HIERBIG, CHK,    NORMAL, YES, ANY, ANY, K_TRI_QUEUED_MEM_CHK},
    {PATH, LARGE,  NONE,    PLAIN,  NORMAL, ANY, ANY, ANY, K_POOL_MEM_S},
    {PATH, LARGE,  NONE,    CHK,    NORMAL, ANY, ANY, ANY, K_POOL_MEM_S_CHK},
    {PATH, LARGE,  NONE,    PLAIN,  WIDE,   ANY, ANY, ANY, K_POOL_MEM},
    {PATH, LARGE,  NONE,    CHK,    WIDE,   ANY, ANY, ANY, K_POOL_MEM_CHK},
    {PATH, LARGE,  ANY,     PLAIN,  ANY,    ANY, ANY, ANY, K_POOL_MEM_TRI},     /* a small mesh, no ring workspace, or out of range */
    {PATH, LARGE,  ANY,     CHK,    ANY,    ANY, ANY, ANY, K_POOL_MEM_TRI_CHK},
    /* ---- trace_path, sphere scenes that fit but stream by preference */
    {PATH, STREAM, NONE,    PLAIN,  NORMAL, ANY, ANY, ANY, K_POOL_MEM_S},
    {PATH, STREAM, NONE,    CHK,    NORMAL, ANY, ANY, ANY, K_POOL_MEM_S_CHK},
    {PATH, STREAM, NONE,    REFR,   NORMAL, ANY, ANY, YES, K_REFR_POOL_MEM},
    {PATH, STREAM, NONE,    REFR,   NORMAL, ANY, ANY, NO,  K_REFR},
    /* ---- trace_path, staged scenes: spheres only */
    {PATH, STAGED, NONE,    PLAIN,  NORMAL, ANY, ANY, ANY, K_TILES},            /* the headline: BASELINE configs 1, 2, 4 */
    {PATH, STAGED, NONE,    CHK,    NORMAL, ANY, ANY, ANY, K_CHK},
    {PATH, STAGED, NONE,    REFR,   NORMAL, ANY, ANY, YES, K_REFR_POOL},
    {PATH, STAGED, NONE,    REFR,   NORMAL, ANY, ANY, NO,  K_REFR},
    {PATH, STAGED, NONE,    PLAIN,  WIDE,   ANY, ANY, ANY, K_BIG},
    {PATH, STAGED, NONE,    CHK,    WIDE,   ANY, ANY, ANY, K_BIG_CHK},
    {PATH, STAGED, NONE,    REFR,   WIDE,   ANY, ANY, ANY, K_BIG_REFR},
    /* ---- ... with a small mesh (flat filter + fp32 pre-test): BASELINE config 3 */
    {PATH, STAGED, FLAT,    PLAIN,  ANY,    ANY, ANY, ANY, K_TRI},
    {PATH, STAGED, FLAT,    CHK,    ANY,    ANY, ANY, ANY, K_TRI_CHK},
    {PATH, STAGED, FLAT,    REFR,   ANY,    ANY, ANY, YES, K_TRI_REFR_POOL},
    {PATH, STAGED, FLAT,    REFR,   ANY,    ANY, ANY, NO,  K_TRI_REFR},
    /* ---- ... with a mesh through the hierarchy: parked walks (BASELINE config 5), else the lane-waiting kernels */
    {PATH, STAGED, HIER,    PLAIN,  NORMAL, YES, YES, ANY, K_TRI_QUEUED_SPH},
    {PATH, STAGED, HIER,    PLAIN,  NORMAL, YES, NO,  ANY, K_TRI_QUEUED},
    {PATH, STAGED, HIER,    CHK,    NORMAL, YES, YES, ANY, K_TRI_QUEUED_CHK_SPH},
    {PATH, STAGED, HIER,    CHK,    NORMAL, YES, NO,  ANY, K_TRI_QUEUED_CHK},
    {PATH, STAGED, HIER,    REFR,   NORMAL, YES, YES, YES, K_TRI_QUEUED_REFR_SPH},
    {PATH, STAGED, HIER,    REFR,   NORMAL, YES, NO,  YES, K_TRI_QUEUED_REFR},
    {PATH, STAGED, HIER,    PLAIN,  ANY,    ANY, ANY, ANY, K_TRI_BIG},          /* no ring workspace, or out of range */
    {PATH, STAGED, HIER,    CHK,    ANY,    ANY, ANY, ANY, K_TRI_BIG_CHK},
    {PATH, STAGED, HIER,    REFR,   ANY,    ANY, ANY, ANY, K_TRI_BIG_REFR},     /* ... or sums / pool that do not fit */
};

static bool pt_row_matches(const PtPickRow &r, const PtPickKey &k)
{
  auto ok = [](int row, int key) { return row == ANY || row == key; };
  /* mesh: a row that asks for HIER takes HIERBIG scenes too (a big mesh is a hierarchy mesh); one that asks for HIERBIG only those */
  const bool mesh_ok = r.mesh == ANY || r.mesh == k.mesh || (r.mesh == HIER && k.mesh == HIERBIG);
  return ok(r.integ, k.integ) && ok(r.stage, k.stage) && mesh_ok && ok(r.mat, k.mat) && ok(r.range, k.range) && ok(r.park, k.park) &&
         ok(r.round, k.round) && ok(r.fit, k.fit);
}

/* what a launch adds to the scene's content when the kernel is picked (pt_plan_launch fills it in) */
struct PtPickFacts
{
  uint32_t integrator;
  int32_t samples, max_depth; /* samples: per sample chunk */
  bool have_park_ws;          /* the parked-walk kernels' ring workspace exists on the device */
  bool wide_pend_ok;          /* the pending-ray pool can be had at 4 x 512 stacks per slot */
  int32_t launch_samples;     /* samples per pixel of the whole launch (all chunks): with max_emission, the fixed-point scale */
  double max_emission;        /* max |emission component| over all materials (pt_acc_scale_exp) */
};

PtPickKey pt_classify(const PtSceneView &scene, const PtPickFacts &f)
{
  PtPickKey k;
  const bool cast = f.integrator == 1u;
  k.integ = cast ? CAST : PATH;
  k.stage = !pt_geom_in_lds(scene) ? LARGE : ((!cast && pt_stream_sized(scene)) ? STREAM : STAGED);
  k.range = scene.wide_range ? WIDE : NORMAL;
  if (scene.n_triangles == 0u)
    k.mesh = NONE;
  else if (pt_filter_in_lds(scene))
    k.mesh = FLAT;
  else
    k.mesh = (scene.n_triangles > PT_FILT_LDS_MAX && scene.n_bvh_nodes != 0u) ? HIERBIG : HIER;
  if (cast)
    k.mat = scene.any_mirror_glass ? GLASS2 : PLAIN;
  else
    k.mat = scene.any_refract ? REFR : (scene.any_checker ? CHK : PLAIN);
  /* sums: the fixed-point pixel sums resolve this launch's terms finely enough (pt_fixed_sums_fit), or the scene takes the
   * unbounded sums of the REFR rows -- their bodies carry the plain and checker code -- like a scene with M_REFRACTION */
  if (!cast && !pt_fixed_sums_fit(f.max_emission, f.launch_samples, f.max_depth))
    k.mat = REFR;
  /* the parked-walk body's conditions: a ring workspace, references that fit the walk's 24-bit stack entries (range: the rows) */
  k.park = (f.have_park_ws && scene.n_bvh_nodes < (1u << 23) && scene.n_triangles < (1u << (23 - PT_BVH_COUNT_BITS))) ? YES : NO;
  k.round = scene.mesh_round ? YES : NO;
  /* the pooled refraction kernels' windowed sums hold 2^31 pieces per word: a sample of a refractive scene has at most
   * 2^(max_depth + 2) - 1 terms (a full binary tree of children), so a chunk needs samples x 2^(max_depth + 1) <= 2^30
   * (pt_refr_pool_fits); and no term may reach 2^128 (pt_window_terms_fit) */
  k.fit = (pt_refr_pool_fits(f.samples, f.max_depth) && pt_window_terms_fit(f.max_emission, f.max_depth) &&
           (k.mesh < HIER || f.wide_pend_ok)) ? YES : NO;
  return k;
}

#ifdef PT_DEV_KERNELS
/* development builds (-DPT_DEV_KERNELS: `make shim-dev` -> librt_hip_dev.so): RT_HIP_KERNEL_VARIANT,
 * read once per process, rewrites the key so that a scene takes another arm of the table (A/B), or names the literal kernel:
 *   0 pt_render_tiles_v0 (the plainest statement of the algorithm)   2 hierarchy scenes on the lane-waiting kernels (park = NO)
 *   3 scenes beyond the staging budget on the static in-memory kernel  4 ... on the compare-form pooled kernel
 *   5 sphere scenes that would stream by preference are staged          7 refractive scenes on the static kernels (fit = NO) */
int pt_dev_variant()
{
  static const int v = [] {
    const char *e = getenv("RT_HIP_KERNEL_VARIANT");
    return (e && e[0] >= '0' && e[0] <= '7' && e[0] != '1' && e[0] != '6') ? e[0] - '0' : 1;
  }();
  return v;
}
static int pt_dev_pick(PtPickKey &k)
{
  const int v = pt_dev_variant();
  if (v == 0 && k.integ == PATH && k.stage != LARGE && k.mat != REFR)
    return K_V0;
  if (v == 2)
    k.park = NO;
  if (v == 3 && k.integ == PATH && k.stage == LARGE)
    return K_MEM;
  if (v == 4 && k.integ == PATH && k.stage == LARGE && k.mesh == NONE && k.mat != REFR)
    return k.mat == CHK ? K_POOL_MEM_CHK : K_POOL_MEM;
  if (v == 5 && k.stage == STREAM)
    k.stage = STAGED;
  if (v == 7)
    k.fit = NO;
  return -1;
}
#endif

static int pt_pick_kernel(const PtSceneView &scene, const PtPickFacts &f)
{
  PtPickKey k = pt_classify(scene, f);
#ifdef PT_DEV_KERNELS
  {
    const int dev = pt_dev_pick(k);
    if (dev >= 0)
      return dev;
  }
#endif
  for (const PtPickRow &r : pt_pick_table)
    if (pt_row_matches(r, k))
      return r.kernel;
  return -1; /* unreachable: the table's last rows of every (integ, stage, mesh) block match ANY of the rest -- pinned by tests/test_pick_table.py */
}

/* ---- how a launch runs: its kernel, the sample chunks that kernel runs and the pools it needs, decided HERE ----------------------
 * rt_hip_render_tiles_chunked, rt_hip_suggest_chunks_depth, rt_hip_kernel_name and rt_hip_kernel_for_class ask pt_plan_launch and
 * re-decide nothing.  In this order:
 *   1. a trace_path launch of a scene with M_REFRACTION that was given a chunk workspace gets at least as many chunks as the
 *      windowed sums of the pooled / parked-walk forms need (pt_refr_chunk_floor) -- the image does not depend on the chunk
 *      count, and the workspace's size does not either; without a workspace it keeps its one chunk, and where that does not fit
 *      the table's fit = NO row (the static kernel of the family) renders it;
 *   2. a trace_path launch of a scene without M_REFRACTION whose fixed-point sums do not fit (pt_fixed_sums_fit) would take the
 *      windowed chunk record, six times the plain one its caller may have sized the workspace for
 *      (rt_hip_scene_chunk_workspace_bytes): it renders its samples in one chunk;
 *   3. the kernel: pt_pick_kernel for the samples of one chunk;
 *   4. a kernel that does not take chunks (the static bodies: cast_ray, the fit = NO rows of M_REFRACTION) runs one -- the pick
 *      of step 3 stays the one made for the chunks asked for.
 * Host arithmetic only, no HIP call: it runs on every launch, and without a device. */
PtPlan pt_plan_launch(const PtSceneView &scene, const PtPlanAsk &a)
{
  const bool trace_path = a.integrator != 1u;
  uint32_t chunks = a.sample_chunks > 1u ? a.sample_chunks : 1u;
  if (trace_path && a.have_chunk_ws)
  {
    const uint32_t need = pt_refr_chunk_floor(scene, a.samples, a.max_depth, a.tile_count);
    if (need > chunks)
      chunks = need;
  }
  if (trace_path && !scene.any_refract && !pt_fixed_sums_fit(a.max_emission, a.samples, a.max_depth))
    chunks = 1u;
  const int32_t samples_per_chunk = (int32_t)(((int64_t)a.samples + chunks - 1) / chunks);
  const PtPickFacts facts = {a.integrator, samples_per_chunk, a.max_depth, a.have_park_ws, a.wide_pend_ok, a.samples, a.max_emission};
  PtPlan p = {};
  p.kernel = pt_pick_kernel(scene, facts);
  if (p.kernel < 0)
    return p; /* unreachable (pt_pick_kernel); pt_launch_render refuses it */
  const PtKernelInfo &k = pt_kernels[p.kernel];
  p.sample_chunks = k.has(CHUNKS) ? chunks : 1u;
  p.windowed = k.has(WINDOWED);
  p.mixed = k.has(MIXED);
  p.queued = k.has(QUEUED);
  if (k.has(PEND_POOL))
  {
    p.pend_entries = pt_pend_entries(scene, a.integrator, a.max_depth);
    p.pend_columns = k.pend_columns();
  }
  return p;
}

const char *pt_kernel_name_of(int which) { return pt_kernels.name_of(which); }
int pt_kernel_count(void) { return K_COUNT; }
unsigned long long pt_kernel_launches(int which) { return pt_kernels.launches(which); } /* rt_hip_kernel_launches */

/* slots per XCD a pool must offer so that every resident workgroup of the kernels that take one finds a slot: CUs per XCD x
 * the most workgroups of any such kernel a CU holds (occupancy without dynamic LDS: an upper bound), + 25 %.  Until round 5
 * these were constants sized for 32 CUs x 4 workgroups with no slack (round-4 advisor finding). */
uint32_t pt_pool_slots_per_xcd(bool park_pool)
{
#ifdef PT_DEV_KERNELS
  { /* development builds: RT_HIP_POOL_SLOTS=n fixes both pools at n slots per XCD (n = 1: acquisition fails for all but eight workgroups) */
    const char *e = getenv("RT_HIP_POOL_SLOTS");
    const unsigned long n = e ? strtoul(e, nullptr, 10) : 0ul;
    if (n >= 1ul && n <= 4096ul)
      return (uint32_t)n;
  }
#endif
  int dev = 0, cus = 256;
  if (hipGetDevice(&dev) == hipSuccess)
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  int most = 1;
  for (int k = 0; k < K_COUNT; k++)
  {
    if (!pt_kernels[k].has(park_pool ? QUEUED : PEND_POOL))
      continue;
    int n = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, reinterpret_cast<const void *>(pt_kernels[k].fn), PT_BLOCK, 0) == hipSuccess)
      most = max(most, n);
    else
      (void)hipGetLastError();
  }
  if (most > 8)
    most = 8; /* 2,048 threads per CU */
  const uint32_t per_xcd = ((uint32_t)cus + PT_PARK_XCDS - 1u) / PT_PARK_XCDS;
  const uint32_t want = per_xcd * (uint32_t)most;
  return ((want + want / 4u) + 31u) & ~31u;
}

/* The camera-dependent tables of a scene for one near_R (two ~2 us kernels): the packed-fp32
 * filter table and the fp32 hierarchy nodes.  The shim keeps them per (scene, near_R) and builds
 * them once (rt_hip_shim.hip, TableSet), never while a render that reads them can be in flight. */
hipError_t pt_launch_build_hull_flags(const double *tri_geom, const double *tri_normal, uint32_t n_tri, double tau,
                                      uint32_t *tri_object, hipStream_t stream)
{
  if (n_tri == 0 || n_tri > PT_HULL_MAX_TRIS)
    return hipSuccess;
  hipLaunchKernelGGL(pt_build_hull_flags, dim3((n_tri + 255u) / 256u), dim3(256), 0, stream, tri_geom, tri_normal, n_tri, tau,
                     tri_object);
  return hipGetLastError();
}

hipError_t pt_launch_build_tables(const PtSceneView &scene, double near_R, float *filt, float *bvh_nodes, hipStream_t stream)
{
  const uint32_t n_nodes = scene.n_bvh_nodes;
  /* every primitive gets a filter entry: small-scene kernels scan triangles through the flat
   * filter, the others read the sphere part only and walk the hierarchy for the triangles */
  const uint32_t n_entries = scene.n_spheres + scene.n_triangles;
  const uint32_t blocks = n_entries ? min(1024u, (n_entries + 255u) / 256u) : 0u;
  if (blocks)
    hipLaunchKernelGGL(pt_build_filter, dim3(blocks), dim3(256), 0, stream, scene.entry_src, n_entries, near_R, filt);
  if (n_nodes)
    hipLaunchKernelGGL(pt_build_bvh, dim3(min(1024u, (n_nodes + 255u) / 256u)), dim3(256), 0, stream, scene.bvh_src,
                       n_nodes, near_R, bvh_nodes);
  /* the pre-test table behind the pair table: in scan order for small scenes (staged in LDS with the pairs), in the
   * hierarchy's leaf order for large meshes (read from HBM at the leaves) */
  if (scene.n_triangles != 0 && (pt_filter_in_lds(scene) || n_nodes != 0))
    hipLaunchKernelGGL(pt_build_tri32, dim3(min(1024u, (scene.n_triangles + 255u) / 256u)), dim3(256), 0, stream,
                       pt_filter_in_lds(scene) ? scene.tri_geom : scene.tri_geom_leaf, scene.n_triangles, near_R,
                       filt + 2 * (size_t)pt_filt_pair_slots(n_entries));
  return hipGetLastError();
}

/* One launch of a kernel that stages the scene in dynamic LDS (workgroups of PT_BLOCK threads).  Beyond 64 KB the kernel's
 * limit is raised first.  The attribute belongs to the (kernel, current device) pair: set whenever it is needed -- a
 * process-wide "already raised" note would skip devices 1..N-1 of the multi-device path (round-2 advisor finding). */
template <class... Params, class... Args>
static hipError_t launch_staged(void (*fn)(Params...), uint32_t blocks, size_t lds_bytes, hipStream_t stream, const Args &...args)
{
  if (lds_bytes > 64 * 1024)
  {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    if (e != hipSuccess)
      return e;
  }
  hipLaunchKernelGGL(fn, dim3(blocks), dim3(PT_BLOCK), lds_bytes, stream, args...);
  return hipGetLastError();
}

hipError_t pt_launch_render(const PtLaunch &launch, hipStream_t stream, int which)
{
  if (!pt_kernels.valid(which))
    return hipErrorInvalidValue;
  size_t extra_lds = 0;
#ifdef PT_DEV_KERNELS
  /* development knob: RT_HIP_EXTRA_LDS=<bytes> of unused dynamic LDS per workgroup, to measure how a
   * kernel responds to fewer resident workgroups per CU */
  static const size_t extra_lds_env = [] {
    const char *e = getenv("RT_HIP_EXTRA_LDS");
    return e ? (size_t)strtoul(e, nullptr, 10) : (size_t)0;
  }();
  extra_lds = extra_lds_env;
#endif
  size_t lds_bytes = pt_render_lds_bytes(launch.scene) + extra_lds;
  const PtKernelInfo &k = pt_kernels[which];
  const PtKernelFn kernel = launch.slot_list ? k.fn_list : k.fn;
  if (k.has(STAGES_NONE))
    lds_bytes = extra_lds; /* the in-memory pooled kernels stage nothing, whatever the scene's size */
  if (k.has(PEND_POOL) && (launch.pend_ws == nullptr || launch.pend_entries < pt_pend_entries(launch.scene, launch.integrator, launch.max_depth) ||
                      launch.pend_slot_doubles < (uint64_t)launch.pend_entries * PT_PEND_FIELDS_HOST * k.pend_columns()))
    return hipErrorInvalidValue; /* a kernel with a pending-ray stack needs its pool, wide enough (rt_hip_shim.hip: pend_pool_for) */
  const bool queued = k.has(QUEUED);
  if (queued && (launch.park_ws == nullptr || launch.park_slots_per_xcd == 0u))
    return hipErrorInvalidValue; /* the parked-walk kernels never run without their workspace (pt_pick_kernel: park) */
  if (launch.sample_chunks > 1 && !k.has(CHUNKS))
    return hipErrorInvalidValue;
  if (queued) /* the spheres' filter pairs (staged forms), then per-lane traversal stacks (24-bit entries) sized by the tree, after the staged scene */
    lds_bytes += (k.has(STAGES_NONE) ? (size_t)0 : (size_t)pt_filt_pair_slots(launch.scene.n_spheres) * 8u) +
                 (((size_t)max(launch.scene.bvh_depth, 1u) * PT_BLOCK * 3u + 15u) & ~(size_t)15u);
  if (launch.acc_keep && (k.has(CHUNKS) ? launch.acc_ws == nullptr || (launch.acc_windows != 0u) != k.has(WINDOWED) : launch.slice_ws == nullptr))
    return hipErrorInvalidValue; /* a pass of an accumulation adds to the sums its caller holds: they are neither cleared nor resolved here */
  /* a mixed grid: a member that takes one, whole slots and chunked slots both, chunks to split into, one-shot, no list */
  if (launch.n_whole != 0u && (!k.has(MIXED) || launch.n_whole >= launch.tile_count || launch.sample_chunks < 2u || launch.acc_keep || launch.slot_list))
    return hipErrorInvalidValue;
  const uint32_t n_chunked = launch.tile_count - launch.n_whole; /* slots that run as sample chunks, if any does: they own the workspace */
  if (launch.sample_chunks > 1 && !launch.acc_keep)
  {
    if ((launch.acc_windows != 0u) != k.has(WINDOWED) || launch.acc_ws == nullptr)
      return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(launch.acc_ws, 0, (size_t)n_chunked * (k.has(WINDOWED) ? PT_ACC_WS_WORDS_WIN : PT_ACC_WS_WORDS) * sizeof(unsigned long long), stream);
    if (e != hipSuccess)
      return e;
  }
  /* a pass over a set of the frame's slots (PtLaunch.slot_list): only an accumulation has sums that outlive the launch */
  if ((launch.slot_list != nullptr) != (launch.slot_count != 0u) || (launch.slot_list && !launch.acc_keep) || launch.slot_count > launch.tile_count)
    return hipErrorInvalidValue;
  /* the parked-walk kernels render a tile per wave, four work units per workgroup */
  const uint32_t n_units = launch.n_whole + (launch.slot_list ? launch.slot_count : n_chunked) * launch.sample_chunks;
  hipError_t e = launch_staged(kernel, queued ? (n_units + PT_BLOCK / 64 - 1) / (PT_BLOCK / 64) : n_units, lds_bytes, stream, launch);
  if (e == hipSuccess && launch.sample_chunks > 1 && !launch.acc_keep)
    e = launch_staged(pt_resolve_tiles, n_chunked, 0, stream, launch, static_cast<const uint32_t *>(nullptr));
  if (e == hipSuccess)
    pt_kernels.launched(which);
  return e;
}

bool pt_kernel_takes_chunks(int which) { return pt_kernels.valid(which) && pt_kernels[which].has(CHUNKS); }

uint32_t pt_resident_workgroups(int which, const PtSceneView &scene)
{
  if (!pt_kernels.valid(which))
    return 0u;
  const PtKernelInfo &k = pt_kernels[which];
  int dev = 0, cus = 0, n = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
      hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, reinterpret_cast<const void *>(k.fn), PT_BLOCK,
                                                   k.has(STAGES_NONE) ? (size_t)0 : pt_render_lds_bytes(scene)) != hipSuccess)
  {
    (void)hipGetLastError();
    return 0u;
  }
  return cus > 0 && n > 0 ? (uint32_t)cus * (uint32_t)n : 0u;
}

hipError_t pt_launch_resolve(const PtLaunch &launch, const uint32_t *tile_samples, hipStream_t stream, int which)
{
  if (!pt_kernels.valid(which) || launch.tile_count == 0u || launch.samples < 1)
    return hipErrorInvalidValue;
  if (pt_kernels[which].has(CHUNKS))
  {
    if (launch.acc_ws == nullptr || (launch.acc_windows != 0u) != pt_kernels[which].has(WINDOWED))
      return hipErrorInvalidValue;
    hipLaunchKernelGGL(pt_resolve_tiles, dim3(launch.tile_count), dim3(PT_BLOCK), 0, stream, launch, tile_samples);
  }
  else
  {
    if (launch.slice_ws == nullptr)
      return hipErrorInvalidValue;
    hipLaunchKernelGGL(pt_resolve_slices, dim3(launch.tile_count), dim3(PT_BLOCK), 0, stream, launch, tile_samples);
  }
  return hipGetLastError();
}

hipError_t pt_launch_tile_error(const float *cur, const float *prev, int width, int height, uint32_t tile_first, uint32_t tile_stride,
                                uint32_t tile_count, float *error, hipStream_t stream)
{
  const uint32_t tiles_x = ((uint32_t)width + PT_TILE - 1) / PT_TILE, waves = PT_BLOCK / 64u;
  hipLaunchKernelGGL(pt_tile_error, dim3((tile_count + waves - 1u) / waves), dim3(PT_BLOCK), 0, stream, cur, prev, width, height, tiles_x,
                     tile_first, tile_stride, tile_count, error);
  return hipGetLastError();
}

hipError_t pt_launch_tile_freeze(const float *error, double threshold, int dilate, uint8_t *keep, uint32_t *tile_samples, int width,
                                 int height, uint32_t tile_first, uint32_t tile_stride, uint32_t tile_count, uint32_t done,
                                 uint32_t *slot_list, uint32_t *live_count, hipStream_t stream)
{
  const uint32_t tiles_x = ((uint32_t)width + PT_TILE - 1) / PT_TILE, tiles_y = ((uint32_t)height + PT_TILE - 1) / PT_TILE;
  if (error) /* else the caller has put its own mask into keep */
    hipLaunchKernelGGL(pt_tile_keep, dim3((tile_count + 255u) / 256u), dim3(256), 0, stream, error, tile_samples, tiles_x, tiles_y, tile_first,
                       tile_stride, tile_count, threshold, dilate, keep);
  hipLaunchKernelGGL(pt_tile_compact, dim3(1), dim3(PT_COMPACT_THREADS), 0, stream, keep, tile_samples, tile_count, done, slot_list, live_count);
  return hipGetLastError();
}

hipError_t pt_launch_selftest_intersect(int kind, const double *rays, const double *prims, const double *entry_src,
                                        float *filt, float *tri32, uint32_t n, double near_R, double filt_shift,
                                        uint8_t *hit, double *tuv, unsigned long long *keep, hipStream_t stream)
{
  if (n == 0)
    return hipSuccess;
  if (kind == 2 && (!PT_MFMA16 || n % 64u != 0u))
    return hipErrorNotSupported; /* a build without the matrix-pipe filter has nothing to test */
  hipLaunchKernelGGL(pt_build_filter, dim3(min(1024u, (n + 255u) / 256u)), dim3(256), 0, stream, entry_src, n, near_R, filt);
  if (kind == 2)
  {
    hipLaunchKernelGGL(pt_selftest_mfma16, dim3(n / 64u), dim3(64), 0, stream, rays, prims, entry_src, reinterpret_cast<const f32x2 *>(filt), n,
                       near_R, near_R * near_R, filt_shift, hit, tuv, keep);
    return hipGetLastError();
  }
  if (kind == 1)
    hipLaunchKernelGGL(pt_build_tri32, dim3((n + 255u) / 256u), dim3(256), 0, stream, prims, n, near_R, tri32);
  hipLaunchKernelGGL(pt_selftest_intersect, dim3((n + 63u) / 64u), dim3(64), 0, stream, kind, rays, prims,
                     reinterpret_cast<const f32x2 *>(filt), reinterpret_cast<const float4 *>(tri32), n, near_R * near_R,
                     filt_shift, 1.7976931348623157e308, hit, tuv, keep);
  return hipGetLastError();
}

/* ---- the AOV kernels: which form a scene takes, and the launch ------------------------------------------------------------ */
int pt_aov_pick(const PtSceneView &scene)
{
  const bool chk = scene.any_checker != 0u;
  if (!pt_geom_in_lds(scene))
    return chk ? A_MEM_CHK : A_MEM;
  const bool tris = scene.n_triangles != 0u;
  if (pt_filter_in_lds(scene))
    return tris ? (chk ? A_TRI_CHK : A_TRI) : (chk ? A_TILES_CHK : A_TILES);
  return tris ? (chk ? A_TRI_BIG_CHK : A_TRI_BIG) : (chk ? A_BIG_CHK : A_BIG);
}

const char *pt_aov_kernel_name_of(int which) { return pt_aov_kernels.name_of(which); }
int pt_aov_kernel_count(void) { return A_COUNT; }
unsigned long long pt_aov_kernel_launches(int which) { return pt_aov_kernels.launches(which); }

hipError_t pt_launch_aov(const PtLaunch &launch, const PtAovOut &out, hipStream_t stream, int which)
{
  if (!pt_aov_kernels.valid(which) || launch.tile_count == 0u)
    return hipErrorInvalidValue;
  /* the staged scene as the beauty kernels stage it (nothing for the in-memory forms) */
  const size_t lds_bytes = which == A_MEM || which == A_MEM_CHK ? 0 : pt_render_lds_bytes(launch.scene);
  const uint32_t waves = PT_BLOCK / 64u; /* a tile per wave */
  const hipError_t e = launch_staged(pt_aov_kernels[which].fn, (launch.tile_count + waves - 1u) / waves, lds_bytes, stream, launch, out);
  if (e == hipSuccess)
    pt_aov_kernels.launched(which);
  return e;
}

/* ---- the ray kernels (query, radiance query, pixel refinement): which of a list's five geometric forms a scene takes ----------
 * One decision for the query list and the sliced table; each gives its own ids (their orders differ). */
static int ray_form_pick(const PtSceneView &scene, int rays, int big, int tri, int tri_big, int mem)
{
  if (!pt_geom_in_lds(scene))
    return mem;
  const bool tris = scene.n_triangles != 0u;
  if (pt_filter_in_lds(scene))
    return tris ? tri : rays;
  return tris ? tri_big : big;
}

/* every form of the sliced kernels pushes pending second children: its pool, as pt_launch_render asks of a
 * PEND_POOL member */
static bool pend_pool_ready(const PtLaunch &launch)
{
  return launch.pend_ws != nullptr && launch.pend_slots_per_xcd != 0u && launch.pend_entries != 0u &&
         launch.pend_entries >= pt_pend_entries(launch.scene, 0u, launch.max_depth) &&
         launch.pend_slot_doubles >= (uint64_t)launch.pend_entries * PT_PEND_FIELDS_HOST * PT_BLOCK;
}

/* ---- the ray-query kernels: which form a scene takes, and the launch ------------------------------------------------------- */
int pt_query_pick(const PtSceneView &scene) { return ray_form_pick(scene, Q_RAYS, Q_BIG, Q_TRI, Q_TRI_BIG, Q_MEM); }

const char *pt_query_kernel_name_of(int which) { return pt_query_kernels.name_of(which); }
int pt_query_kernel_count(void) { return Q_COUNT; }
unsigned long long pt_query_kernel_launches(int which) { return pt_query_kernels.launches(which); }

hipError_t pt_launch_query(const PtLaunch &launch, const PtQuery &query, hipStream_t stream, int which)
{
  if (!pt_query_kernels.valid(which) || query.n == 0u || query.n > 0xFFFFFFFFull)
    return hipErrorInvalidValue;
  const size_t lds_bytes = which == Q_MEM ? 0 : pt_render_lds_bytes(launch.scene); /* the staged scene, as the AOV launch */
  const uint32_t blocks = (uint32_t)((query.n + PT_BLOCK - 1u) / PT_BLOCK); /* at most 2^24 */
  const hipError_t e = launch_staged(pt_query_kernels[which].fn, blocks, lds_bytes, stream, launch, query);
  if (e == hipSuccess)
    pt_query_kernels.launched(which);
  return e;
}

/* ---- the sliced kernels (radiance queries, pixel refinement): which form a scene takes, and the launch ------------------------
 * One pick for both lists (they are the columns of PT_SLICED_FAMILY), one launch behind both launchers: n entries of `list`'s
 * form `which`, 64 entries x 4 sample slices per workgroup.  args_ok: the caller's own argument checks. */
int pt_trace_pick(const PtSceneView &scene) { return ray_form_pick(scene, T_RAYS, T_BIG, T_TRI, T_TRI_BIG, T_MEM); }

template <class List, class Args>
static hipError_t launch_sliced(List &list, int which, bool args_ok, const PtLaunch &launch, const Args &args, hipStream_t stream)
{
#ifdef PT_DIAG
  return hipErrorNotSupported; /* (the diagnostic build counts into stats[4 ..]: a caller's d_stats has RT_HIP_NSTATS words) */
#endif
  if (!list.valid(which) || !args_ok || args.n == 0u || args.n > 0xFFFFFFFFull || launch.samples < 1 || !pend_pool_ready(launch))
    return hipErrorInvalidValue;
  const size_t lds_bytes = which == T_MEM ? 0 : pt_render_lds_bytes(launch.scene); /* the staged scene, as the query launch */
  const uint32_t blocks = (uint32_t)((args.n + PT_SLICED_ENTRIES - 1u) / PT_SLICED_ENTRIES); /* at most 2^26 */
  const hipError_t e = launch_staged(list[which].fn, blocks, lds_bytes, stream, launch, args);
  if (e == hipSuccess)
    list.launched(which);
  return e;
}

const char *pt_trace_kernel_name_of(int which) { return pt_trace_kernels.name_of(which); }
int pt_trace_kernel_count(void) { return T_COUNT; }
unsigned long long pt_trace_kernel_launches(int which) { return pt_trace_kernels.launches(which); }

hipError_t pt_launch_trace(const PtLaunch &launch, const PtTrace &trace, hipStream_t stream, int which)
{
  return launch_sliced(pt_trace_kernels, which, (uint64_t)trace.index_first + trace.n <= 0x100000000ull, launch, trace, stream);
}

const char *pt_pixel_kernel_name_of(int which) { return pt_pixel_kernels.name_of(which); }
int pt_pixel_kernel_count(void) { return T_COUNT; }
unsigned long long pt_pixel_kernel_launches(int which) { return pt_pixel_kernels.launches(which); }

hipError_t pt_launch_pixels(const PtLaunch &launch, const PtPixels &pixels, hipStream_t stream, int which)
{
  const bool args_ok = (uint64_t)pixels.sample_first + (uint64_t)launch.samples <= 0x80000000ull && launch.width >= 2 && launch.height >= 2 &&
                       (uint64_t)launch.width * (uint64_t)launch.height == (uint64_t)pixels.n_pixels;
  return launch_sliced(pt_pixel_kernels, which, args_ok, launch, pixels, stream);
}

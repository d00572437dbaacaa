/* raytracer.h -- the drop-in boundary: the reference's public C API, served by
 * an MI355X (gfx950) path tracer.
 *
 * A caller written against gue-ni/raytracer.c's raytracer.h (its main.c, its
 * test.c) compiles and links against this header + libraytracer_amd.so
 * unchanged: every struct below has the reference's field order, size and
 * offsets (checked against the compiled reference in tests/test_oracle_ref.py:
 * Object 88 B, Camera 96 B, Options 56 B, Ray 48 B, Hit 80 B, Vertex 40 B), and
 * every function the reference's raytracer.o exports is exported here with
 * the same signature (reference raytracer.h:135-164).
 *
 * What is different behind the boundary: render() hands the per-pixel
 * trace_path()/intersect() loop (reference raytracer.c:176-223, 482-554,
 * 393-464, 77-174) to hand-written HIP through the C-ABI in rt_hip.h.  There
 * is no CPU fallback: without a GPU render() reports the HIP error on stderr
 * and exits, as the reference's main.c:415-419 does for its own failures.
 *
 * Build-defined extensions (not in the reference) are grouped at the end and
 * prefixed rt_ / named *_ex.
 */
#ifndef RAYTRACER_H
#define RAYTRACER_H

/* libc headers a caller of the reference's header gets transitively (its main.c and test.c
 * rely on that) */
#include <assert.h>
#include <float.h>
#include <math.h>
#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "vector.h"
#include "rt_hip.h" /* RtHipDenoiseParams (denoise_frame) */

#ifdef __cplusplus
extern "C" {
#endif

/* ---- constants and helper macros (reference raytracer.h:21-56) -------------
 * Same names, same values, same expansions as seen by a caller; in particular the
 * argument-evaluation and NaN behaviour of MAX / MIN / CLAMP, which the tonemap and the
 * Russian roulette depend on, and the CLAMP_BETWEEN quirk. */

#if !defined(PI)
#define PI 3.14159265359 /* the reference's truncated pi; it feeds parity (atan2 texture coordinate) */
#endif
#define EPSILON 1e-8     /* self-intersection / parallel-ray threshold */
#if !defined(MAX_DEPTH)
#define MAX_DEPTH 5      /* default bounce limit; at run time: rt_set_max_depth() */
#endif
#define MONTE_CARLO_SAMPLES 1

#define MAX(a, b) ((a) > (b) ? (a) : (b)) /* NaN in `a` selects b, NaN in `b` selects b */
#define MIN(a, b) ((a) < (b) ? (a) : (b))
#define CLAMP(x) (MAX(0, MIN(x, 1)))      /* hence CLAMP(NaN) == 1: a NaN pixel tonemaps to 255 */
/* Reproduced quirk (reference raytracer.h:30): the first argument is ignored, so the "cosine"
 * refract() clamps is always 1 and its refracted ray goes straight on. */
#define CLAMP_BETWEEN(x, min_v, max_v) (MAX(min_v, MIN(max_v, 1)))
#define ABS(x) ((x < 0) ? (-x) : (x))
#define EQ(a, b) (ABS((a) - (b)) < EPSILON)

/* vec3 / Ray literals; C++ callers get aggregate initialisation instead of compound literals */
#if defined(__cplusplus)
#define VECTOR(x, y, z) (vec3{(x), (y), (z)})
#define RAY(o, d) (Ray{(o), (d)})
#else
#define VECTOR(x, y, z) ((vec3){(x), (y), (z)})
#define RAY(o, d) ((Ray){.origin = o, .direction = d})
#endif
#define RGB(r, g, b) (VECTOR((r) / 255.0, (g) / 255.0, (b) / 255.0)) /* 8-bit components -> [0, 1] */

#define BLACK RGB(0, 0, 0)
#define WHITE RGB(255, 255, 255)
#define RED RGB(255, 0, 0)
#define GREEN RGB(0, 192, 48)
#define BLUE RGB(0, 0, 255)
#define ZERO_VECTOR RGB(0, 0, 0)
#define ONE_VECTOR (VECTOR(1.0, 1.0, 1.0))
#define BACKGROUND RGB(10, 10, 10) /* radiance of a miss AND of a depth-terminated path (raytracer.c:487-490) */
#define RANDOM_COLOR VECTOR(random_double(), random_double(), random_double())

/* material flags (raytracer.h:53-56): one of the first three decides the bounce -- tested in
 * the order M_REFRACTION, M_REFLECTION, else diffuse (raytracer.c:514-545) -- optionally
 * or-ed with M_CHECKERED */
#define M_DEFAULT ((uint)1 << 1)    /* diffuse */
#define M_REFLECTION ((uint)1 << 2) /* perfect mirror */
#define M_REFRACTION ((uint)1 << 3) /* the reference's two-child "glass" */
#define M_CHECKERED ((uint)1 << 4)  /* albedo x 0.3 / 0.7 by texture coordinate */

/* ---- types (reference raytracer.h:60-131): field order, sizes and offsets are the ABI ----- */

typedef uint32_t uint;

typedef struct Vertex
{
  vec3 pos; /* offset 0 */
  vec2 tex; /* offset 24; (0, 0) when the OBJ has no vt */
} Vertex;   /* 40 bytes */

typedef struct Ray
{
  vec3 origin;
  vec3 direction; /* unit length except after a mirror bounce (raytracer.c:542) */
} Ray;            /* 48 bytes */

/* Unindexed triangle soup: vertices[3*i .. 3*i+2] is triangle i. */
typedef struct TriangleMesh
{
  size_t num_triangles;
  Vertex *vertices;
} TriangleMesh;

/* The live scene element: a sphere with its material inline. */
typedef struct Object
{
  uint flags;    /* offset  0: M_* */
  double radius; /* offset  8 */
  vec3 center;   /* offset 16 */
  vec3 color;    /* offset 40: albedo, components in [0, 1] */
  vec3 emission; /* offset 64: radiance, may exceed 1 */
} Object;        /* 88 bytes */

typedef struct Hit
{
  double t;       /* ray parameter of the closest hit */
  double u, v;    /* texture coordinates: atan2-based on a sphere, interpolated on a triangle */
  vec3 point;
  vec3 normal;    /* unit; geometric, un-flipped */
  uint object_id; /* index into objects[] */
} Hit;            /* 80 bytes */

typedef struct Camera
{
  vec3 position;
  vec3 horizontal;        /* viewport edge vectors */
  vec3 vertical;
  vec3 lower_left_corner; /* see init_camera: with get_camera_ray's subtraction, row 0 is the top */
} Camera;                 /* 96 bytes */

typedef struct Options
{
  vec3 background; /* unused by render() (BACKGROUND is a macro) */
  char *result;    /* output file name */
  char *obj;       /* mesh file name */
  int width, height, samples;
} Options;         /* 56 bytes */

/* Types the reference declares but no live code path uses (its retired mesh-capable Object,
 * raytracer.h:62-102); kept so that code naming them still compiles. */
typedef struct Material
{
  uint flags;
  vec3 color, emission;
  double ka, ks, kd;
} Material;
typedef struct Sphere
{
  vec3 center;
  double radius;
} Sphere;
typedef union Geometry
{
  TriangleMesh *mesh;
  Sphere *sphere;
} Geometry;
typedef enum GeometryType
{
  GEOMETRY_SPHERE,
  GEOMETRY_MESH,
} GeometryType;

/* ---- the reference's exported functions (raytracer.h:135-164), same signatures ------------- */

/* framebuffer: caller-owned width*height*3 bytes, RGB, row 0 = top.  Blocks until the image is
 * complete; adds the device counters to ray_count and intersection_test_count. */
void render(uint8_t *framebuffer, Object *objects, size_t n_objects, Camera *camera, Options *options);
void init_camera(Camera *camera, vec3 position, vec3 target, Options *options);

/* Host-side single-primitive tests, bit-identical to the device code's. */
bool intersect_sphere(const Ray *ray, vec3 center, double radius, Hit *hit);
bool intersect_triangle(const Ray *ray, Vertex vertex0, Vertex vertex1, Vertex vertex2, Hit *hit);
vec3 calculate_surface_normal(vec3 v0, vec3 v1, vec3 v2); /* normalize(cross(v2 - v0, v1 - v0)) */
vec3 point_at(const Ray *ray, double t);

/* Uniform [0,1) and [min,max) from the host-side stream (rt_set_seed). */
double random_double(void);
double random_range(double min, double max);

vec3 clamp(const vec3 v);
void print_v(const char *msg, const vec3 v);
void print_m(const mat4 m);

/* Declared by the reference (raytracer.h:158) but never defined there; defined
 * here: Wavefront OBJ -> unindexed triangle soup, polygons fan-triangulated,
 * positions read as float then widened (what the reference's vendored
 * tinyobj_loader_c yields), tex = (0,0) where the file has no vt.
 * mesh->vertices is malloc'd; the caller frees it. */
bool load_obj(const char *filename, TriangleMesh *mesh);

extern long long ray_count;               /* trace_path()-equivalent calls */
extern long long intersection_test_count; /* primitive tests */

/* ---- build-defined extensions ----------------------------------------------- */

/* A triangle mesh with a material: the scene element the reference's retired
 * Object layout (raytracer.h:95-102) and commented-out mesh scan
 * (raytracer.c:417-435) describe.  Meshes are scanned after the spheres, in
 * array order, triangles in index order. */
typedef struct
{
  uint flags;
  vec3 color, emission;
  TriangleMesh mesh;
} MeshObject;

/* render() plus meshes and an optional linear output: linear_rgb, if not
 * NULL, receives width*height*3 floats, the per-pixel sample MEAN before the
 * gamma-5 tonemap.  framebuffer may be NULL when only linear_rgb is wanted. */
void render_ex(uint8_t *framebuffer, float *linear_rgb, Object *objects, size_t n_objects,
               MeshObject *meshes, size_t n_meshes, Camera *camera, Options *options);

/* Run-time settings the reference fixes at compile time or takes from libc
 * state.  Defaults: depth MAX_DEPTH (5), seed 1666943821 (main.c:182), 1 GPU. */
void rt_set_max_depth(int max_depth);
void rt_set_seed(uint64_t seed);
void rt_set_devices(int n_devices); /* a host that never calls it: RT_DEVICES=N of the environment, else 1 */
int rt_get_max_depth(void);
uint64_t rt_get_seed(void);

/* Which integrator render() runs -- the reference chooses at compile time with the `#if 1`
 * of raytracer.c:207-211: RT_TRACE_PATH (default) = trace_path (:482-554), RT_CAST_RAY =
 * cast_ray (:556-641, Whitted-style: one point light, Phong, shadow rays, mirror and
 * "refraction" children).  Other values are ignored. */
enum { RT_TRACE_PATH = 0, RT_CAST_RAY = 1 };
void rt_set_integrator(int integrator);
int rt_get_integrator(void);

/* A thin lens for render() / render_ex(): depth of field.  aperture_radius 0 (the default) leaves them on the pinhole path they
 * take without this call, whatever focus_distance is.  With an aperture above 0 the frame is the lens frame of rt_hip.h
 * (rt_hip_render_lens_image: lens rays of radius aperture_radius about the camera position, sharp on the plane focus_distance in
 * front of the camera, traced as radiance queries) on one device, with the path tracer.  The setter only stores the values and
 * refuses nothing: what the shim refuses (a focus_distance that is not positive and finite, RT_CAST_RAY) makes render() fail as
 * it fails for any other refusal.  The defaults are 0 and 1.  Either pointer of the getter may be NULL.
 * The lens frame runs on ONE device whatever rt_set_devices() or RT_DEVICES say, and takes no part in cancellation: the flag of
 * rt_set_cancel_flag() is not polled, the frame is always whole, and rt_last_render_cancelled() reads 0 after it.
 * rt_last_render_seconds() is the whole call by the host's clock, not kernel time. */
void rt_set_lens(double aperture_radius, double focus_distance);
void rt_get_lens(double *aperture_radius, double *focus_distance);

/* The probe-lit preview in render()'s and render_ex()'s place (rt_hip.h, "probe grids"): with nx, ny, nz >= 1 set, they bake a grid
 * of nx x ny x nz light probes over the scene -- on each axis [-reach, reach] about the world's origin, reach = rt_hip_scene_bounds',
 * origin = -reach, step = (2.0 * reach) / (double)(n - 1); an axis of one probe has it at 0 --, options->samples rays a probe at
 * rt_set_max_depth()'s depth under rt_set_seed()'s seed, and write rt_hip_probe_preview_image's frame (one first-hit sample a pixel
 * for the albedo, the default miss colour, no facing weight; made on the one scene whose bounds placed the grid, through
 * rt_hip_probe_preview_scene_image): noise-free and globally lit.  Any count below 1 turns it
 * off (the default).  It goes before rt_set_lens, runs on ONE device and takes no part in cancellation, as the lens frame;
 * ray_count and intersection_test_count grow by the bake's rays.  The reference has no counterpart. */
void rt_set_probe_grid(int nx, int ny, int nz);
void rt_get_probe_grid(int *nx, int *ny, int *nz);

/* The probe grid's visibility weight (rt_hip.h, "probe visibility"): with res in 2 .. 32 the preview above also bakes every probe's
 * depth moments in a res x res octahedral map from the same rays and shades through rt_hip_probe_preview_vis_scene_image, the other
 * fields rt_hip_probe_vis_defaults' for the grid: light no longer leaks through walls thinner than a cell.  0, or any other value,
 * turns it off (the default): the frame is then the plain preview's, bit for bit.  Without a probe grid it does nothing. */
void rt_set_probe_visibility(int res);
int rt_get_probe_visibility(void);

/* A probe grid that follows a moving scene (rt_hip.h, "probe updates").  With rt_set_probe_grid on, rt_set_scene_updates(1) and
 * rays >= 1, render() and render_ex() keep their scene and the grid's state (coefficients, depth moments, ages) between calls.  A call
 * whose scene equals the previous call's but for sphere centres and radii and vertex positions takes those in place; if the grid it
 * derives is the previous call's as well -- the same counts, the same reach, the same visibility resolution -- the frame is one
 * update round of `rays` rays a probe (stride 1, the hysteresis given, round 1, 2, ... counting up from the bake) and the preview lit
 * by the state (rt_hip_probe_update_preview_scene_image), instead of the full bake.  Anything else starts over with the full bake of
 * options->samples rays a probe, which leaves every age at 1: a first call, another scene (changed flags, colours or emission
 * included, unless rt_set_material_updates(1) lets the kept scene take them in place), a changed reach or resolution.
 * rays <= 0 (the default) turns it off: render() is then bit for bit what it is without this call, and keeps nothing.  A hysteresis
 * outside [0, 1) leaves the setting as it was. */
void rt_set_probe_update(int rays, double hysteresis);
void rt_get_probe_update(int *rays, double *hysteresis);

/* Who builds the triangle hierarchy of the scenes render() and its kin upload: RT_BVH_HOST (default) = one host core,
 * RT_BVH_DEVICE = the GPU (rt_hip.h, RT_HIP_BVH_DEVICE).  Images, bytes and counters are the same under either; the time a
 * new or changed scene takes to become renderable is what differs.  Other values are ignored.  The reference has no
 * counterpart: it tests every triangle (raytracer.c:137-150 in a loop). */
enum { RT_BVH_HOST = 0, RT_BVH_DEVICE = 1 };
void rt_set_bvh_builder(int builder);
int rt_get_bvh_builder(void);

/* A deforming mesh, moving spheres.  on != 0: when the scene of a render() call differs from the previous call's only in vertex
 * positions, sphere centres and sphere radii -- the same counts, flags, colours, emissions and tex coordinates, the same size and
 * devices -- the scene kept on the GPU takes them in place (rt_hip.h, rt_hip_scene_update_vertices_host: the triangles' records
 * recomputed and the hierarchy refitted on the device; rt_hip_scene_update_spheres_host: the spheres' records and what the scene
 * derives from them) instead of being rebuilt, so render() in a loop over an animated MeshObject[] or Object[] re-creates nothing.
 * The frame is the one a rebuilt scene gives, bit for bit.  The default, 0: every changed scene is rebuilt.  The CLI renders one
 * frame per process and has no use for it. */
void rt_set_scene_updates(int on);
int rt_get_scene_updates(void);

/* A lamp dimmed, a wall recoloured, a ball turned to glass.  on != 0: the scene of a render() call may also differ from the
 * previous call's in flags, colours and emission (of objects and meshes): the scene kept on the GPU takes them in place (rt_hip.h,
 * rt_hip_scene_update_materials_host: the material records and what the scene derives from them) instead of being rebuilt.
 * Independent of rt_set_scene_updates: a call that changes materials and positions updates in place only where both are on.  Under
 * rt_set_probe_update such a call runs one update round on the kept grid state (the state follows the new light by its hysteresis)
 * instead of the full bake.  The frame of a plain render() is the one a rebuilt scene gives, bit for bit.  The default, 0: a changed
 * material rebuilds the scene, and under rt_set_probe_update starts over with the full bake. */
void rt_set_material_updates(int on);
int rt_get_material_updates(void);

/* Under rt_set_scene_updates(1) a refit keeps the hierarchy's topology, and the walks get dearer as the mesh leaves the shape the
 * tree was built for.  A ratio r >= 1 (finite) makes every frame that is taken as an in-place vertex update end with
 * rt_hip_scene_maintain_bvh(scene, r) on every cached scene: the refitted tree is priced on the device, and rebuilt in place when
 * it costs more than r times what it cost as built (rt_hip.h; DESIGN.md has the measured relation between a ratio and frame
 * time -- there is no recommended value).  0, the default: never.  Another value (NaN, infinite, negative, between 0 and 1) is
 * ignored and the setting stays, as rt_set_bvh_builder ignores an unknown builder.  The frame is the same either way, bit for bit. */
void rt_set_bvh_rebuild_ratio(double max_ratio);
double rt_get_bvh_rebuild_ratio(void);

/* Cooperative cancellation (what the reference's SIGINT handler, main.c:37-48,422, is for):
 * while a flag is registered, long renders poll it between slabs of tiles; when it becomes
 * non-zero render()/render_ex() return early with the finished part of the image in the
 * framebuffer (the rest stays as the caller initialised it / zero) and
 * rt_last_render_cancelled() reports 1.  Set the flag from a signal handler. */
void rt_set_cancel_flag(const volatile int *flag);
int rt_last_render_cancelled(void);

/* Progressive rendering: render_ex's frame (options->samples per pixel, the budget) in passes of pass_samples (the last one may
 * be shorter), on ONE device.  After every pass on_pass (may be NULL) gets the samples done, the budget, the pass's kernel seconds
 * and `user`.  The cancel flag (rt_set_cancel_flag) is polled between passes; at least one pass always runs.  framebuffer and
 * linear_rgb (either may be NULL) receive the whole image of the samples done: after the budget it is the one-shot frame bit for
 * bit (include/rt_hip.h, rt_hip_accum_*); when cancelled, a complete image of fewer samples, and rt_last_render_cancelled()
 * reports 1.  Returns the samples per pixel the image holds, or a negative RT_HIP_E* code with the reason on stderr: more than one
 * device (rt_set_devices), pass_samples < 1, or a failure of the GPU path.  The counters and timings below are those of all passes. */
typedef void RtPassFn(int done, int total, double kernel_seconds, void *user);
int render_progressive(uint8_t *framebuffer, float *linear_rgb, Object *objects, size_t n_objects, MeshObject *meshes,
                       size_t n_meshes, Camera *camera, Options *options, int pass_samples, RtPassFn *on_pass, void *user);

/* Adaptive sampling: render_ex's frame with options->samples as the BUDGET per pixel, on ONE device.  8x8 tiles whose error
 * estimate has settled stop early (include/rt_hip.h, rt_hip_accum_run_adaptive; params == NULL: rt_hip_adapt_defaults); every
 * tile of the frame is, bit for bit, the tile of a uniform frame of that tile's own sample count.  framebuffer and linear_rgb
 * (either may be NULL, not both) receive the image; tile_samples (may be NULL) the count map, ceil(w/8) x ceil(h/8) words,
 * row-major.  After every estimate on_checkpoint (may be NULL) gets the samples done, the budget, the tiles still live and `user`;
 * the cancel flag (rt_set_cancel_flag) is polled there: when cancelled the image holds the samples done and
 * rt_last_render_cancelled() reports 1.  Returns the LARGEST per-tile count, or a negative RT_HIP_E* code with the reason on
 * stderr.  The counters and timings below are those of all passes. */
long long rt_last_pixel_samples(void); /* pixel samples the last render_adaptive rendered (its mean per pixel: / (w * h)) */
typedef void RtCheckpointFn(int done, int total, unsigned live_tiles, void *user);
int render_adaptive(uint8_t *framebuffer, float *linear_rgb, uint32_t *tile_samples, Object *objects, size_t n_objects,
                    MeshObject *meshes, size_t n_meshes, Camera *camera, Options *options, const RtHipAdaptParams *params,
                    RtCheckpointFn *on_checkpoint, void *user);

/* First-hit feature buffers of the frame's own samples (include/rt_hip.h, rt_hip_render_aov_*): options->samples camera samples
 * per pixel with the seed of rt_get_seed(), i.e. the samples render_ex draws its camera rays with.  Row-major arrays of
 * width x height pixels, each may be NULL (not all): albedo and normal 3 floats per pixel (the mean over the samples of the
 * first hit's colour -- checkered where M_CHECKERED -- and unit normal; BACKGROUND and 0 for a sample that misses), depth the
 * least t of the samples that hit (+inf: none), object_id the object that gave it (spheres 0..n_objects-1, then meshes;
 * 0xFFFFFFFF: none), hits how many samples hit.  Runs on one device, the first of the device map.  Returns the samples per
 * pixel, or a negative RT_HIP_E* code with the reason on stderr. */
typedef struct
{
  float *albedo, *normal, *depth;
  uint32_t *object_id, *hits;
} RtAovImage;
int render_aov(RtAovImage *out, Object *objects, size_t n_objects, MeshObject *meshes, size_t n_meshes, Camera *camera,
               Options *options);

/* Closest hits of the caller's own rays (include/rt_hip.h, rt_hip_query_rays_host: the contract in full): for each of the n rays,
 * used as given, what intersect() (raytracer.c:393-464; here: the spheres, then the meshes in array order) finds with hit->t =
 * DBL_MAX on entry, as a hit iff its t < t_max[i] (t_max NULL: DBL_MAX for every ray).  status[i] (may be NULL): 1 hit, 0 miss,
 * 2 invalid ray (a non-finite component, a direction whose squared length is farther than 2^-13 from 1, a NaN limit).  hits[i] of a
 * hit holds t, point, normal and object_id (spheres 0 .. n_objects-1, then meshes) as the reference's arithmetic gives them, bit
 * for bit, and u, v, the texture coordinates of the WINNER, computed on the host: spheres as raytracer.c:410-411 (libm's atan2),
 * triangles the :154-167 interpolation of the vertices' tex with the winner's barycentrics.  (The literal scan leaves in u, v what
 * the last passing triangle wrote, closest or not: a documented difference.)  Any other ray: t = DBL_MAX, object_id = 0xFFFFFFFF,
 * the rest 0.  Runs on one device, the first of the device map.  Returns 0, or a negative RT_HIP_E* code with the reason on stderr. */
int intersect_rays(const Ray *rays, size_t n, const double *t_max, Object *objects, size_t n_objects, MeshObject *meshes,
                   size_t n_meshes, Hit *hits, uint8_t *status);

/* What light arrives along the caller's own rays (include/rt_hip.h, rt_hip_trace_rays_host: the contract in full): for each of the n
 * rays, used as given, radiance[i] = the mean of `samples` trace_path() samples (raytracer.c:482-554) at rt_get_max_depth(), sample s
 * of ray i on the stream (rt_get_seed(), i, s) after render()'s two jitter draws.  status[i] (may be NULL): 1 traced, 2 invalid ray (a
 * non-finite component, a direction whose squared length is farther than 2^-13 from 1: radiance 0).  Adds the traced paths and their
 * primitive tests to ray_count and intersection_test_count, as render does.  Runs on one device, the first of the device map.
 * Returns 0, or a negative RT_HIP_E* code with the reason on stderr. */
int trace_rays(const Ray *rays, size_t n, int samples, Object *objects, size_t n_objects, MeshObject *meshes, size_t n_meshes,
               vec3 *radiance, uint8_t *status);

/* Edge-avoiding a-trous denoise of a frame (include/rt_hip.h, rt_hip_denoise: the contract in full) guided by the first-hit
 * buffers of its own samples: linear_in is the frame's linear mean (render_ex's linear_rgb, width x height x 3 floats), aov its
 * render_aov buffers (normal, depth and hits always; albedo with RT_HIP_DENOISE_DEMODULATE, object_id with _OBJECT_EDGES).
 * Writes the denoised linear image to linear_out and its tonemapped bytes to framebuffer (either may be NULL, not both; linear_out
 * may be linear_in).  params NULL: rt_hip_denoise_defaults.  Runs on one device, the first of the device map.  Returns 0, or a
 * negative RT_HIP_E* code with the reason on stderr. */
int denoise_frame(uint8_t *framebuffer, float *linear_out, const float *linear_in, const RtAovImage *aov, int width, int height,
                  const RtHipDenoiseParams *params);

/* Temporal reprojection of a frame onto the history of the frames before it (include/rt_hip.h, rt_hip_reproject: the contract in
 * full): linear_in is the frame's linear mean (render_ex's linear_rgb), aov its render_aov buffers (normal, depth, hits and
 * object_id), camera its camera; hist_linear and hist_len are the previous call's linear_out and len_out, hist_aov and hist_camera
 * the previous frame's buffers and camera (all four NULL: the first frame).  Writes the accumulated linear image to linear_out
 * (it may be linear_in) and the history length per pixel to len_out (both required), the tonemapped bytes to framebuffer and the
 * motion in pixels (2 floats per pixel) to motion_out (either may be NULL).  params NULL: rt_hip_reproject_defaults.  The scene
 * must not have changed between the two frames.  Runs on one device, the first of the device map.  Returns 0, or a negative
 * RT_HIP_E* code with the reason on stderr. */
int reproject_frame(uint8_t *framebuffer, float *linear_out, float *len_out, float *motion_out, const float *linear_in,
                    const RtAovImage *aov, const Camera *camera, const float *hist_linear, const float *hist_len,
                    const RtAovImage *hist_aov, const Camera *hist_camera, int width, int height, const RtHipReprojectParams *params);

/* Guided upsampling of a low-resolution frame to full size (include/rt_hip.h, rt_hip_upsample: the contract in full): linear_low is
 * the low frame's linear mean (render_ex's linear_rgb at low_width x low_height under the FULL frame's camera, denoised or not),
 * aov_low its render_aov buffers, aov the render_aov buffers of the width x height frame (normal, depth and hits always; albedo with
 * RT_HIP_UPSAMPLE_DEMODULATE, object_id with _OBJECT_EDGES).  Writes the full-size linear image to linear_out, its tonemapped bytes
 * to framebuffer and the confidence per pixel (1 .. 0: how much of the bilinear weight found the pixel's surface; 0: plain
 * bilinear; -1: nothing usable) to conf_out; each may be NULL.  params NULL: rt_hip_upsample_defaults.  Runs on one device, the
 * first of the device map.  Returns 0, or a negative RT_HIP_E* code with the reason on stderr. */
int upsample_frame(uint8_t *framebuffer, float *linear_out, float *conf_out, const float *linear_low, const RtAovImage *aov_low,
                   int low_width, int low_height, const RtAovImage *aov, int width, int height, const RtHipUpsampleParams *params);

/* Kernel-only wall time of the last render()/render_ex(), seconds, and the
 * count of scene casts (rays that ran the intersection scan). */
double rt_last_render_seconds(void);
long long rt_last_ray_bounces(void);

#ifdef __cplusplus
}
#endif

#endif /* RAYTRACER_H */

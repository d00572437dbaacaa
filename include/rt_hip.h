/* rt_hip.h -- C-ABI of the MI355X (gfx950) path-tracing shim, librt_hip.so.
 *
 * This is the drop-in boundary for the reference's hot path: everything
 * render() (gue-ni/raytracer.c raytracer.c:176-223) does per pixel --
 * get_camera_ray :375-384, trace_path :482-554, intersect :393-464,
 * intersect_sphere :77-118, intersect_triangle :120-174,
 * calculate_surface_normal :42-45, the sampling RNG :227-253, reflect /
 * checkered_texture / refract :349-391, sample accumulation and the gamma-5
 * tonemap :212-220 -- runs on the device behind the entry points below.
 * Plain C: pointers and sizes only, no C++ or torch types, no exceptions.
 * The reference has no FFI layer of its own (its API is raytracer.h); the
 * host library libraytracer_amd.so implements raytracer.h on top of this
 * header, and INTEGRATION.md shows the binding a maintainer of the reference
 * would add to call it directly.
 *
 * Conventions
 *   - every function returns 0 on success or a negative RT_HIP_E* code;
 *     rt_hip_last_error() gives the message (thread-local).
 *   - "d_" pointers are device memory on the scene's device; "h_" are host.
 *   - a stream argument is a hipStream_t passed as void* (NULL = the null
 *     stream); calls taking a stream are asynchronous on it.
 *   - there is NO CPU fallback anywhere: without a usable GPU every entry
 *     point that needs one fails with RT_HIP_ENODEV.
 *
 * Image decomposition: the image is cut into 8x8-pixel tiles, numbered
 * row-major (tiles_x = ceil(width/8)).  One call renders the tiles
 *     t = tile_first + k * tile_stride,  k = 0 .. tile_count-1
 * into a COMPACT tile-major buffer: tile k occupies floats
 * [k*192, (k+1)*192) as 64 pixels (row-major inside the tile) x RGB.  With
 * tile_first = rank, tile_stride = world size this is the interleaved
 * multi-GPU partition; rt_hip_untile() scatters a (gathered) compact buffer
 * back to a row-major image.  Pixels of edge tiles that fall outside the
 * image are written as zeros and skipped by rt_hip_untile().
 */
#ifndef RT_HIP_H
#define RT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RT_HIP_TILE 8        /* tile edge, pixels */
#define RT_HIP_TILE_PIXELS 64

enum
{
  RT_HIP_OK = 0,
  RT_HIP_ENODEV = -1,   /* no usable HIP device */
  RT_HIP_EINVAL = -2,   /* bad argument */
  RT_HIP_ENOMEM = -3,   /* host or device allocation failed */
  RT_HIP_ERUNTIME = -4, /* a HIP / RCCL runtime call failed */
  RT_HIP_ELIMIT = -5,   /* scene exceeds what the kernel supports */
  RT_HIP_ECANCELLED = -6, /* rt_hip_render_image stopped early on the cancel flag; output is partial */
};

/* Layout-identical to the reference's Object (raytracer.h:104-111): 88 bytes. */
typedef struct
{
  uint32_t flags; /* M_DEFAULT 2 | M_REFLECTION 4 | M_REFRACTION 8, | M_CHECKERED 16 */
  double radius;
  double center[3];
  double color[3];
  double emission[3];
} RtHipSphere;

/* Layout-identical to the reference's Vertex (raytracer.h:61): 40 bytes. */
typedef struct
{
  double pos[3];
  double tex[2];
} RtHipVertex;

/* A triangle mesh with its material (the MeshObject extension of
 * include/raytracer.h; reference raytracer.h:77-81 + :95-102).
 * vertices: host pointer, 3*num_triangles entries, unindexed. */
typedef struct
{
  uint32_t flags;
  double color[3];
  double emission[3];
  size_t num_triangles;
  const RtHipVertex *vertices;
} RtHipMesh;

/* Layout-identical to the reference's Camera (raytracer.h:121-124): 96 bytes. */
typedef struct
{
  double position[3];
  double horizontal[3];
  double vertical[3];
  double lower_left_corner[3];
} RtHipCamera;

typedef struct
{
  int32_t width, height; /* pixels */
  int32_t samples;       /* per pixel (Options.samples) */
  int32_t max_depth;     /* the reference's compile-time MAX_DEPTH (raytracer.h:25) */
  uint64_t seed;         /* stream key, see rt_rng.h */
  uint32_t tile_first, tile_stride, tile_count;
  uint32_t integrator;   /* RT_HIP_TRACE_PATH (0, the default) or RT_HIP_CAST_RAY */
} RtHipParams;

/* The two sides of the `#if 1` in the reference's render() (raytracer.c:207-211): the path
 * tracer trace_path (:482-554), which is what the reference ships, and cast_ray (:556-641),
 * the Whitted-style integrator it keeps compiled next to it (one fixed point light, Phong
 * shading, shadow rays, mirror / "refraction" children; no random draws beyond the camera
 * jitter).  With RT_HIP_CAST_RAY, RT_HIP_STAT_RAYS counts cast_ray calls (:558) and
 * RT_HIP_STAT_CASTS counts scene scans, i.e. the primary and the shadow scan of every hit. */
enum
{
  RT_HIP_TRACE_PATH = 0,
  RT_HIP_CAST_RAY = 1
};

/* counters accumulated (+=) by a render call */
enum
{
  RT_HIP_STAT_RAYS = 0,  /* reference ray_count: trace_path calls (raytracer.c:484) */
  RT_HIP_STAT_CASTS = 1, /* rays that ran the scene scan = "ray-bounces" */
  RT_HIP_STAT_TESTS = 2, /* reference intersection_test_count (raytracer.c:79,122) */
  RT_HIP_STAT_SAMPLES = 3,
  RT_HIP_NSTATS = 4
};

typedef struct RtHipScene RtHipScene; /* opaque, device-resident */

/* ---- device / errors ---------------------------------------------------------- */

int rt_hip_device_count(void);
const char *rt_hip_last_error(void);
/* name and compute-unit count of a device (name_cap bytes incl. NUL) */
int rt_hip_device_info(int device, char *name, size_t name_cap, int *compute_units);

/* ---- scene: replaces the Object[] argument of render() ------------------------- */

/* Uploads spheres and meshes to `device` in the kernel's layout.  Object ids
 * follow the reference's scan order: spheres 0..n_spheres-1, then meshes. */
int rt_hip_scene_create(const RtHipSphere *spheres, size_t n_spheres, const RtHipMesh *meshes,
                        size_t n_meshes, int device, RtHipScene **out_scene);
void rt_hip_scene_destroy(RtHipScene *scene);

/* Who builds the triangle hierarchy of a scene.  RT_HIP_BVH_HOST: the recursive binned builder on one host core (BvhBuild,
 * csrc/bvh_build.h), the default.  RT_HIP_BVH_DEVICE: the capped full-sweep surface-area builder on the device
 * (csrc/bvh_device.hip): three per-axis sorted lists, every admissible split position of every axis priced, level by level; the
 * tree is a deterministic function of the triangles (BvhSweep in csrc/bvh_build.h states it in sequential C++, and the device's
 * nodes and order equal it byte for byte).  A hierarchy only decides WHICH triangles get the exact test: frames, bytes and
 * counters are the same under either builder; the build time and the walks' cost are what differ.
 * Both have the same limits: fewer than 2^27 triangles, leaves of at most 15, the least depth such leaves allow.  The device
 * builder's workspace (about 360 bytes a triangle and the sort's temporaries, freed before the call returns) that cannot be had is RT_HIP_ENOMEM, never a
 * silent host build. */
enum
{
  RT_HIP_BVH_HOST = 0,
  RT_HIP_BVH_DEVICE = 1
};
typedef struct RtHipSceneOptions
{
  uint32_t struct_size; /* sizeof(RtHipSceneOptions), set by rt_hip_scene_options_defaults() */
  uint32_t bvh_builder; /* RT_HIP_BVH_HOST (default) or RT_HIP_BVH_DEVICE */
} RtHipSceneOptions;
void rt_hip_scene_options_defaults(RtHipSceneOptions *opts);
/* rt_hip_scene_create with options; opts == NULL or the defaults: rt_hip_scene_create itself.  A struct_size below the
 * struct's or an unknown builder is RT_HIP_EINVAL, reported before any device is looked at. */
int rt_hip_scene_create_opts(const RtHipSphere *spheres, size_t n_spheres, const RtHipMesh *meshes, size_t n_meshes, int device,
                             const RtHipSceneOptions *opts, RtHipScene **out_scene);
/* The hierarchy of a scene (any out pointer may be NULL): the builder that made it, its depth (levels that hold an inner node),
 * the least depth leaves of 15 allow, its node count, and its expected walk cost -- evaluated on the host from the downloaded
 * nodes in node order by BvhBuild::tree_cost()'s formula.  A scene without triangles reports 0 nodes and a cost of 0. */
int rt_hip_scene_bvh_info(const RtHipScene *scene, uint32_t *builder, uint32_t *depth, uint32_t *max_depth, uint32_t *n_nodes,
                          double *tree_cost);
/* Downloads the fp64 source nodes (n_nodes x 16 doubles: two child boxes, two refs in the 13th, padding) and the leaf order
 * (one triangle index per triangle); either may be NULL.  For tests and tools/bvh_sim.py. */
int rt_hip_scene_bvh_read(const RtHipScene *scene, double *h_nodes, uint32_t *h_order);
/* seconds the hierarchy build of this scene took: the host builder by the host's clock, the device builder by device events
 * around its kernels */
double rt_hip_scene_bvh_build_seconds(const RtHipScene *scene);

/* ---- a tree priced on the device ----
 * rt_hip_scene_bvh_info's tree_cost downloads every node (128 bytes each); this evaluates the same formula where the nodes lie
 * (k_tree_cost, csrc/scene_update.hip; the terms are csrc/bvh_build.h's bvh_cost_*) and reads back 8 bytes.  Synchronous, on the
 * null stream of the scene's device.
 * CONTRACT: the cost is a pure function of the bytes of the fp64 source nodes (n_nodes x 16 doubles, rt_hip_scene_bvh_read's
 * layout; n0 = node 0), all arithmetic fp64, unfused, in the order written:
 *   root      lo[k] = fmin(n0[k], n0[6 + k]), hi[k] = fmax(n0[3 + k], n0[9 + k]) for k = 0, 1, 2; a_root = half_area(lo, hi) with
 *             half_area = dx * dy + dy * dz + dz * dx, d = hi - lo.  n_nodes == 0, or !(a_root > 0) || !(a_root < 1e300): the cost
 *             is 0.0.
 *   terms     node i: (c0 + c1); c_k = +0.0 where child k is an empty leaf (leaf flag set, count 0), otherwise
 *             (half_area(child k's box) / a_root) * (leaf ? 45.0 * count : 60.0), count = the ref's low 4 bits.
 *   sum       in blocks of 256 terms, missing terms +0.0: for m = 128, 64, ..., 1: v[i] = v[i] + v[i + m] for i < m (the shape
 *             rt_hip_tile_error states); v[0] is the block's sum.  The block sums are the next level's terms, reduced by the same
 *             rule, level after level, until one value `total` is left.  cost = 60.0 + total.
 * No atomic takes part and no workgroup waits for another (the levels are launched one after another), so the same bytes give the
 * same cost on every run.  It differs from rt_hip_scene_bvh_info's node-order sum by rounding alone: at most
 * n_nodes * 2^-52 * cost, both being sums of 2 n_nodes non-negative terms.
 * TOTAL: any node bytes have a defined result -- NaN boxes, inverted boxes, refs that point nowhere (a ref is only read for its
 * flag and count; no child is followed).  A NaN in one of the root's two boxes gives way to the other box's component (fmin /
 * fmax); a root area that is NaN, zero, negative or >= 1e300 prices the tree at 0.0; otherwise a NaN or infinite term makes the
 * cost NaN or infinite by IEEE addition in the order above (a NaN result's sign and payload are not specified).
 * rt_hip_scene_bvh_cost: the scene's current tree (refitted, if it was); a scene without triangles: 0.0.  RT_HIP_EINVAL: a NULL
 * argument.  RT_HIP_ERUNTIME: an unusable scene.  RT_HIP_ENOMEM: the workspace (8 bytes per 256 nodes; made at the
 * first call and kept with the scene, so a per-frame question allocates nothing).
 * rt_hip_bvh_cost_nodes_host: the same for n_nodes nodes in host memory, staged on `device` (logical, as in rt_hip_scene_create)
 * -- for tools, and for tests of the reduction's edges.  Arguments are checked before a device is looked for: a NULL cost, NULL
 * nodes with n_nodes > 0 or n_nodes >= 2^27 is RT_HIP_EINVAL, then a missing device RT_HIP_ENODEV.  n_nodes == 0 needs no
 * device: 0.0. */
int rt_hip_scene_bvh_cost(const RtHipScene *scene, double *cost);
int rt_hip_bvh_cost_nodes_host(const double *h_nodes, size_t n_nodes, int device, double *cost);

/* ---- the topology rebuilt in place ----
 * rt_hip_scene_rebuild_bvh runs the device builder (RT_HIP_BVH_DEVICE above) over the scene's current triangles -- they are on the
 * device already, and after any number of vertex updates equal a fresh scene's bit for bit -- and installs the new tree in the
 * scene the handle names.  Synchronous.
 * CONTRACT: after the call the nodes and order of rt_hip_scene_bvh_read, the leaf-ordered geometry, rt_hip_scene_bvh_info (the
 * builder becomes RT_HIP_BVH_DEVICE, whoever built the scene), rt_hip_kernel_name, the frames, bytes and counters of every launch
 * and the ray queries equal, byte for byte, those of a scene freshly created with RT_HIP_BVH_DEVICE from the same positions.
 * Spheres, materials, triangle records, hull bits, bounds, the parked-walk workspace and every handle stay.
 * The new tree's node count may differ from the old one's.  A scene keeps a node capacity (the count it was created with, or the
 * largest a rebuild has needed since): a tree that fits is written in place; one that does not gets a side allocation for the
 * source nodes and the first table set's fp32 nodes (192 bytes a node), kept until the scene is destroyed or a later rebuild
 * needs a larger one.  Table sets beyond the first are freed (the next launch that needs one allocates it at the new size);
 * every table set is stale and rebuilt by the next launch, as after an update; the level array of the refit is dropped and made
 * again by the next vertex update.
 * Refusals, every one before the first write into the scene (the build writes its own workspace alone), so the scene is
 * unchanged: RT_HIP_EINVAL -- a NULL scene; a scene without triangles; an RtHipAccum on the scene that has not been destroyed; a
 * launch of the scene being submitted on another thread.  RT_HIP_ERUNTIME -- an unusable scene; an inconsistency the builder
 * found in its own result.  RT_HIP_ENOMEM -- the builder's workspace (about 360 bytes a triangle) or the side allocation.
 * RT_HIP_ELIMIT -- a depth above the traversal stack (24; it cannot occur at an unchanged triangle count).  A HIP runtime failure
 * after installing has begun is RT_HIP_ERUNTIME and leaves the scene UNUSABLE, as a failed update does.
 * rt_hip_scene_rebuild_info (any out pointer may be NULL): how many rebuilds the scene has taken (rt_hip_scene_update_info keeps
 * counting updates alone), the host-clock seconds of the last one, and built_cost -- rt_hip_scene_bvh_cost of the tree as it was
 * last BUILT: taken at every rebuild, and for a created scene at the first request (this call, rt_hip_scene_maintain_bvh) or
 * before its first vertex update refits the tree, whichever comes first; 0.0 without triangles. */
int rt_hip_scene_rebuild_bvh(RtHipScene *scene);
int rt_hip_scene_rebuild_info(const RtHipScene *scene, uint64_t *rebuilds, double *last_seconds, double *built_cost);

/* The decision: prices the current (refitted) tree on the device, reports *cost_ratio = cost / built_cost (1.0 where built_cost
 * is 0: nothing to compare), and rebuilds iff cost_ratio > max_ratio (*rebuilt = 1; else 0).  After a rebuild the next call
 * reports 1.0.  There is no default ratio: what a ratio costs in frame time depends on the scene and the view ("Keeping
 * a deforming mesh's tree good", has a measured table to choose from).  RT_HIP_EINVAL: max_ratio NaN, infinite or below 1 (checked
 * first); a NULL scene; a scene without triangles.  Otherwise rt_hip_scene_bvh_cost's and rt_hip_scene_rebuild_bvh's errors; a
 * refusal of the rebuild leaves the scene as it was, and *cost_ratio is set even then.  Either out pointer may be NULL. */
int rt_hip_scene_maintain_bvh(RtHipScene *scene, double max_ratio, double *cost_ratio, int *rebuilt);

/* ---- a deforming mesh: new vertex positions for a scene that exists ----
 * New positions for every triangle of the scene: 9 doubles a triangle (v0, v1, v2), in scene triangle order (mesh by mesh).
 * d_positions: device memory on the scene's device, not inside the scene (from skinning, a cloth step, a torch tensor);
 * h_positions: host memory, staged by the call.  Synchronous: returns when the scene is ready, and the next launch of any
 * kernel sees the new geometry.  Every per-triangle record is recomputed on the device by the operations scene creation uses,
 * and the existing hierarchy is REFITTED: same topology, same leaf order, new boxes (BvhRefit, csrc/bvh_build.h).  A hierarchy
 * only decides which triangles get the exact test, so frames, bytes and counters after an update equal those of a scene
 * freshly created from the same positions; only the walks' cost can drift as the mesh leaves the shape the tree was built for
 * (rt_hip_scene_bvh_cost prices the refitted tree on the device; rt_hip_scene_maintain_bvh compares it with the tree as built and
 * rt_hip_scene_rebuild_bvh gives the scene a new topology in place when it has drifted too far: all above).  The
 * parked-walk workspace, the table sets' storage and every handle stay.  Spheres, triangle counts, materials and tex
 * coordinates do not change; the topology is not rebuilt.
 * RT_HIP_EINVAL, with the scene unchanged: n_triangles differs from the scene's count; a scene without triangles; a NULL
 * pointer; d_positions not device memory of the scene's device, or inside the scene; an RtHipAccum on the scene that has not
 * been destroyed (its plan holds the scene as it was); a launch of the scene being submitted on another thread; a position
 * that is not finite (|vertex| <= 1e300, rt_hip_scene_create's rule).  RT_HIP_ENOMEM, with the scene unchanged: the workspace
 * (256 bytes; the host form adds the staged positions; the first update adds 4 bytes a node, kept with the scene).
 * A HIP runtime failure after writing has begun is RT_HIP_ERUNTIME and leaves the scene UNUSABLE: every later launch or update
 * on it returns RT_HIP_ERUNTIME, and only rt_hip_scene_destroy is allowed.
 * The caller must not launch on the scene from another thread during the call; work submitted before it is waited for. */
int rt_hip_scene_update_vertices(RtHipScene *scene, const double *d_positions, size_t n_triangles);
int rt_hip_scene_update_vertices_host(RtHipScene *scene, const double *h_positions, size_t n_triangles);
/* how many updates the scene has taken -- of any kind: vertices, spheres or materials -- and the host-clock seconds of the last
 * one; either may be NULL */
int rt_hip_scene_update_info(const RtHipScene *scene, uint64_t *updates, double *last_seconds);
/* for tests: tri_geom (9n), tri_normal (3n), the triangles' entry_src records (6n), tri_object (n, hull bits included); any may be NULL */
int rt_hip_scene_read_triangles(const RtHipScene *scene, double *geom, double *normal, double *entry, uint32_t *object);
/* for tests: the triangles' bounding sphere (radius < 0: no triangles), the scene's reach (>= |p| for every point of a primitive
 * of ordinary size: what near_R is made of) and whether a launch takes the _sph members; any may be NULL */
int rt_hip_scene_bounds(const RtHipScene *scene, double mesh_center[3], double *mesh_radius, double *reach, uint32_t *mesh_round);

/* ---- moving spheres: new centres and radii for a scene that exists ----
 * d_spheres / h_spheres: 4 doubles a sphere (cx, cy, cz, radius) for EVERY sphere of the scene, in object order -- the layout of
 * rt_hip_selftest_intersect kind 0.  d_spheres: device memory on the scene's device, not inside the scene (a particle system, a
 * physics step that keeps its state in a torch tensor); h_spheres: host memory, staged by the call.  Synchronous, as the vertex
 * update is.  One streaming kernel (k_update_spheres, csrc/scene_update.hip), a thread a sphere, rewrites the spheres' entry_src
 * records and their geom4 copy and reduces what a scene derives from its spheres -- the spheres' part of the reach, the largest
 * |centre|, the wide-range flag -- by maxima alone; the leading wall-sized spheres (whole pairs, at most 8) come from the first 8
 * records.  scene_sphere_bounds (csrc/scene_spheres.h; the text stands in csrc/bvh_build.h) is the one text of all of it, shared with rt_hip_scene_create.  Then every table set is stale and
 * rebuilt in place by the next launch.  Materials, flags, counts, meshes, object ids and every handle stay (materials and flags
 * have an update of their own, rt_hip_scene_update_materials).
 * CONTRACT: after an update the records, the scalars (rt_hip_scene_sphere_bounds, rt_hip_scene_bounds), rt_hip_kernel_name and the
 * frames, bytes and counters of every launch equal, bit for bit, those of a scene freshly created from the same spheres.  A move may
 * change the wide-range flag or the number of leading walls, and with them the kernel a launch picks: that is intended, and why a
 * live RtHipAccum refuses the update.
 * Acceptance is rt_hip_scene_create's: |radius| outside [1e-100, 1e100] (or NaN) is RT_HIP_ELIMIT; any centre is taken.
 * RT_HIP_EINVAL: a NULL pointer; n_spheres differs from the scene's count; a scene without spheres; d_spheres not device memory of
 * the scene's device, or inside the scene; an RtHipAccum on the scene that has not been destroyed; a launch of the scene being
 * submitted on another thread.  RT_HIP_ENOMEM: the workspace (256 bytes; the host form adds the staged spheres).  After each of these
 * the scene is unchanged: the kernel's first run writes nothing of the scene.  A scene that an earlier update left unusable:
 * RT_HIP_ERUNTIME.  A HIP runtime failure after writing has begun is RT_HIP_ERUNTIME and leaves the scene UNUSABLE, as above. */
int rt_hip_scene_update_spheres(RtHipScene *scene, const double *d_spheres, size_t n_spheres);
int rt_hip_scene_update_spheres_host(RtHipScene *scene, const double *h_spheres, size_t n_spheres);
/* for tests: entry_src's sphere records (6n doubles), geom4 (4n); either may be NULL */
int rt_hip_scene_read_spheres(const RtHipScene *scene, double *entry, double *geom4);
/* for tests: what the scene derives from its spheres -- the spheres' part of the reach, max |centre|, the wide-range flag a launch
 * reads, the leading walls (n_big of them, whole pairs; big_r / big_c are 0 from n_big on); any may be NULL */
int rt_hip_scene_sphere_bounds(const RtHipScene *scene, double *reach_spheres, double *max_center, uint32_t *wide_range, uint32_t *n_big,
                               double big_r[8], double big_c[8]);

/* ---- changing materials: new colours, emission and (optionally) flags for a scene that exists ----
 * d_materials / h_materials: 6 doubles an object (colour r g b, emission r g b) for EVERY object of the scene in
 * rt_hip_scene_create's numbering -- the spheres in their order, then mesh m at n_spheres + m.  d_flags / h_flags: one uint32 an
 * object (M_DEFAULT 2 | M_REFLECTION 4 | M_REFRACTION 8, | M_CHECKERED 16), or NULL: every object keeps the flags it has.
 * d_*: device memory on the scene's device, not inside the scene; h_*: host memory, staged by the call.  Synchronous, as the other
 * updates are.  One streaming kernel (k_update_materials, csrc/scene_update.hip), a thread an object, rewrites the `material`
 * records (prob, albedo / prob, emission, flags) and the color_raw triples and reduces what a scene derives from its materials:
 * the largest |emission component| (a maximum) and three flag classes (ORs) -- an M_REFRACTION material, an M_CHECKERED one, one
 * with M_REFLECTION and M_REFRACTION.  scene_material_bounds (csrc/scene_materials.h; the text stands in csrc/bvh_build.h) is the
 * one text of all of it, shared with rt_hip_scene_create.  The table sets hold filter records, fp32 nodes and tri32 records, made
 * of positions alone: they STAY VALID, and the next launch builds nothing.  Geometry, counts, meshes, object ids and every handle
 * stay.
 * CONTRACT: after an update the records and scalars (rt_hip_scene_read_materials, rt_hip_scene_material_bounds), rt_hip_kernel_name
 * for every integrator, the query, trace and AOV kernel names, and the frames, bytes and counters of every launch equal, bit for
 * bit, those of a scene freshly created from the same data -- where "bit for bit" takes a NaN of a record as equal to a NaN: a
 * black colour gives prob = 0 and 0 * (1 / 0) = NaN in doubles 1..3 of its record, whose sign bit is the machine's default (the
 * host's at creation, the device's after an update); no kernel reads the three (the reference's `random_double() < prob` never
 * holds for prob = 0), so no output can differ.  An update may change a flag class or the largest emission, and with them the
 * kernel a launch picks and the scale of its fixed-point sums: that is intended, and why a live RtHipAccum refuses the update.
 * Histories (temporal reprojection, previews) hold radiance of the old materials: reset them after an update.
 * Acceptance is rt_hip_scene_create's: a colour component that is negative, above 1e100 or NaN, or an |emission component| above
 * 1e100 or NaN, is RT_HIP_EINVAL (-0.0 is accepted).  Also RT_HIP_EINVAL: a NULL d_materials; n_objects differs from n_spheres +
 * n_meshes; a scene without objects; d_materials or d_flags not device memory of the scene's device, or inside the scene; an
 * RtHipAccum on the scene that has not been destroyed; a launch of the scene being submitted on another thread.  RT_HIP_ENOMEM: the
 * workspace (256 bytes; the host form adds the staged input).  After each of these the scene is unchanged: the kernel's first run
 * writes nothing of the scene.  A scene that an earlier update left unusable: RT_HIP_ERUNTIME.  A HIP runtime failure after writing
 * has begun is RT_HIP_ERUNTIME and leaves the scene UNUSABLE, as above. */
int rt_hip_scene_update_materials(RtHipScene *scene, const double *d_materials, const uint32_t *d_flags, size_t n_objects);
int rt_hip_scene_update_materials_host(RtHipScene *scene, const double *h_materials, const uint32_t *h_flags, size_t n_objects);
/* for tests: the `material` records (8n doubles: prob, albedo / prob, emission, the flags as the uint64 bit pattern of double 7)
 * and color_raw (3n), n = n_spheres + n_meshes; either may be NULL */
int rt_hip_scene_read_materials(const RtHipScene *scene, double *material, double *color_raw);
/* for tests: what the scene derives from its materials -- the largest |emission component| and the three flag classes a launch
 * reads; any may be NULL */
int rt_hip_scene_material_bounds(const RtHipScene *scene, double *max_emission, uint32_t *any_refract, uint32_t *any_checker,
                                 uint32_t *any_mirror_glass);
/* for tests: the scene's one device allocation (what "inside the scene" means to the updates' refusals); either may be NULL */
int rt_hip_scene_memory(const RtHipScene *scene, const void **base, size_t *bytes);

int rt_hip_scene_device(const RtHipScene *scene);
size_t rt_hip_scene_primitives(const RtHipScene *scene); /* spheres + triangles */
/* diagnostic: how many triangles the scene marked as HULL FACETS -- every triangle of the scene lies on the inner
 * side of their plane, the stored normal (calculate_surface_normal, raytracer.c:42-45) pointing outward (*n_plus)
 * or inward (*n_minus).  A bounce that leaves such a facet on its outer side cannot meet a triangle, so the
 * hierarchy kernels do not walk it (pt_device.h).  0 / 0 for more than 65,536 triangles (the marking is quadratic). */
int rt_hip_scene_hull_facets(const RtHipScene *scene, uint32_t *n_plus, uint32_t *n_minus);
/* name of the render kernel a launch of this scene takes (the family is picked by scene content:
 * triangles, table size, M_CHECKERED / M_REFRACTION materials) -- for profiles and bench lines */
const char *rt_hip_kernel_name(const RtHipScene *scene, uint32_t integrator);

/* ... and of the kernel the calling thread's last rt_hip_render_tiles / _chunked call actually launched: the launch's own
 * facts (samples x depth against the windowed sums of the M_REFRACTION kernels, the width of the pending-ray pool that could
 * be had) can name another row of the pick table than the scene alone does. */
const char *rt_hip_last_launch_kernel(void);

/* The kernel family by index (0 .. rt_hip_kernel_count() - 1): name, and how many render launches of it this PROCESS has
 * made (*launches, may be NULL) -- what a test run actually exercised.  NULL beyond the family. */
int rt_hip_kernel_count(void);
const char *rt_hip_kernel_launches(int index, uint64_t *launches);

/* The pick table itself, without a device: which kernel a launch of a scene of this class takes.  A class is what the family is
 * split by (pt_kernel.hip, pt_pick_table): counts decide staging and the mesh form, the flags the material code. */
typedef struct
{
  uint32_t integrator;              /* RT_HIP_TRACE_PATH | RT_HIP_CAST_RAY */
  uint32_t n_spheres, n_meshes, n_triangles;
  uint32_t any_checker, any_refract, any_mirror_glass; /* materials: M_CHECKERED, M_REFRACTION, M_REFLECTION | M_REFRACTION on one object */
  uint32_t wide_range;              /* a centre or radius beyond 1e17 */
  uint32_t mesh_round;              /* the triangles' bounding sphere is no larger a target than their box */
  int32_t samples_per_chunk, max_depth;
  uint32_t have_park_ws;            /* the parked-walk workspace could be allocated */
  uint32_t wide_pend_ok;            /* the pending-ray pool could be had at 4 x 512 stacks per slot */
  double max_emission;              /* max |emission component| over all materials: with samples_per_chunk (taken as the
                                     * launch's samples) and max_depth, whether the fixed-point pixel sums resolve the launch;
                                     * where they do not, trace_path takes the M_REFRACTION forms' unbounded sums */
} RtHipSceneClass;
const char *rt_hip_kernel_for_class(const RtHipSceneClass *scene_class);

/* Device-side failures of the render launches on `device` since the last call: sticky bits, read and cleared here.  A
 * workgroup that cannot get a slot of a per-device pool renders nothing; its tile reads NaN (bytes 255) -- which is also what
 * a legitimate NaN sample gives (raytracer.c:218-220), so the pixel values cannot tell the caller: this can.  Call it after
 * synchronising the streams launched on.  Returns RT_HIP_OK with *flags = 0, or RT_HIP_ERUNTIME with the reason in
 * rt_hip_last_error().  rt_hip_render_image() checks it itself and returns the error. */
enum
{
  RT_HIP_FAIL_PEND_SLOT = 1, /* no free slot in the pending-ray pool (two-child materials) */
  RT_HIP_FAIL_PARK_SLOT = 2  /* no free slot in the parked-walk workspace (mesh hierarchies) */
};
int rt_hip_launch_status(int device, uint32_t *flags);

/* ---- the hot path: replaces the loop nest of render() (raytracer.c:184-222) ---- */

/* d_tiles_rgb : tile_count*192 floats  (linear per-pixel sample mean)
 * d_tiles_rgb8: tile_count*192 bytes   (gamma-5 tonemap, raytracer.c:218-220); may be NULL
 * d_stats     : RT_HIP_NSTATS uint64 accumulators; may be NULL */
int rt_hip_render_tiles(const RtHipScene *scene, const RtHipCamera *camera, const RtHipParams *params,
                        float *d_tiles_rgb, uint8_t *d_tiles_rgb8, uint64_t *d_stats, void *stream);

/* The same render with every tile's samples split over `sample_chunks` workgroups (finer
 * work units: matters when a GPU holds few tiles, e.g. 1/8 of a 1080p frame).  Partial sums
 * are exact integers, so the image is bit-identical for every sample_chunks.  d_workspace:
 * rt_hip_chunk_workspace_bytes(tile_count) bytes of device memory (may be NULL when
 * sample_chunks == 1); it is cleared, filled and resolved on `stream`.
 * rt_hip_suggest_chunks() returns a good value for the scene's device. */
size_t rt_hip_chunk_workspace_bytes(uint32_t tile_count);   /* enough for any scene */
/* ... for this scene: scenes without M_REFRACTION need a sixth of it (plain fixed-point sums; the others keep windowed sums).
 * A launch of such a scene whose fixed-point sums would be too coarse (an emitter bright for its samples and depth) takes the
 * M_REFRACTION forms' unbounded sums and renders in one chunk, whatever sample_chunks asks: the image is the same. */
size_t rt_hip_scene_chunk_workspace_bytes(const RtHipScene *scene, uint32_t tile_count);
uint32_t rt_hip_suggest_chunks(const RtHipScene *scene, uint32_t tile_count, int32_t samples);
/* ... knowing the launch's max_depth: scenes with M_REFRACTION need samples_per_chunk x 2^(max_depth + 1) <= 2^30 for the pooled
 * and parked-walk kernels (their windowed pixel sums) -- the suggestion is at least that many chunks.  A launch that gets fewer
 * (or no workspace) and does not fit runs on the static kernel of the family, three times slower on a glass mesh: the image is
 * the same.  rt_hip_render_tiles_chunked raises a too-small chunk count itself whenever a workspace was handed over. */
uint32_t rt_hip_suggest_chunks_depth(const RtHipScene *scene, uint32_t tile_count, int32_t samples, int32_t max_depth);
int rt_hip_render_tiles_chunked(const RtHipScene *scene, const RtHipCamera *camera, const RtHipParams *params,
                                uint32_t sample_chunks, void *d_workspace, float *d_tiles_rgb,
                                uint8_t *d_tiles_rgb8, uint64_t *d_stats, void *stream);

/* ---- progressive rendering: one frame accumulated over passes ------------------------------------------------------------
 * An accumulation renders the frame of params->samples samples per pixel (the BUDGET) in passes of any sizes, and can be resolved
 * after any pass into the mean of the samples done so far.  The frame after the whole budget is BIT-IDENTICAL to the one-shot
 * frame, whatever the passes were: what rt_hip_render_tiles_chunked gives for the same parameters at
 * rt_hip_suggest_chunks_depth(budget) chunks (tiles, bytes and the summed counters); and two accumulations of the same frame agree
 * bit for bit at every sample count both have reached.  A sample's value depends only on its (seed, pixel, sample) stream
 * (rt_rng.h), and the pixel sums are exact integers (fixed point, or windowed words) or fp64 slice sums added in the one-shot order.
 *   - The plan is made ONCE, at create: pt_plan_launch for the whole budget with a chunk workspace and the suggested chunks, with
 *     the fallback rows of a one-shot launch (no parked-walk workspace, no wide pending-ray pool) and the budget's fixed-point
 *     scale.  Every pass runs that member with those sums; rt_hip_accum_kernel names it.
 *   - Create allocates the frame's sums -- tile_count x 9,240 bytes for windowed sums (the M_REFRACTION forms), x 1,560 for
 *     fixed-point ones, x 6,144 (3 x 256 fp64 slice sums) for the static body; at 1080p about 300 / 50 / 200 MB -- and, where the
 *     member needs one, a pending-ray pool of its own, and holds them until destroy.  The scene (and with it the parked-walk
 *     workspace) must outlive the accumulation.
 *   - rt_hip_accum_add renders the next `samples` samples of every pixel (asynchronous on `stream`; d_stats: RT_HIP_NSTATS
 *     accumulators, += per pass, may be NULL -- over all passes they sum to the one-shot counters).  samples <= 0 or more than the
 *     budget has left: RT_HIP_EINVAL, nothing changes.  The passes of one accumulation must run in order (one stream, or
 *     synchronised between them).
 *   - rt_hip_accum_resolve writes the mean of the samples done so far into a compact tile buffer (as rt_hip_render_tiles);
 *     asynchronous on `stream`, which must be ordered after the passes.  rt_hip_accum_read_image is the synchronous row-major form
 *     for C hosts (waits for the device, either output may be NULL; pixels of tiles outside the accumulation's tile set are 0)
 *     and checks the device's status word (rt_hip_launch_status). */
typedef struct RtHipAccum RtHipAccum; /* opaque */
int rt_hip_accum_create(const RtHipScene *scene, const RtHipCamera *camera, const RtHipParams *params, RtHipAccum **out_accum);
int rt_hip_accum_add(RtHipAccum *accum, int32_t samples, uint64_t *d_stats, void *stream);
int rt_hip_accum_resolve(const RtHipAccum *accum, float *d_tiles_rgb, uint8_t *d_tiles_rgb8, void *stream); /* mean of samples done */
int rt_hip_accum_read_image(const RtHipAccum *accum, float *h_rgb, uint8_t *h_rgb8);
/* rt_hip_accum_add for C hosts: on the null stream, synchronous; h_stats (RT_HIP_NSTATS, may be NULL) += the pass's counters,
 * kernel_seconds (may be NULL) = the pass's device time */
int rt_hip_accum_add_host(RtHipAccum *accum, int32_t samples, uint64_t *h_stats, double *kernel_seconds);
int32_t rt_hip_accum_samples(const RtHipAccum *accum); /* samples per pixel done */
const char *rt_hip_accum_kernel(const RtHipAccum *accum);
void rt_hip_accum_destroy(RtHipAccum *accum);

/* ---- adaptive sampling: converged tiles stop early, the frame stays bit-exact ------------------------------------------------
 * An accumulation can FREEZE tiles between passes: a frozen tile takes no further samples, the passes that follow render the live
 * tiles only, and a resolve divides every tile by its own sample count.  Freezing is monotone -- a frozen tile never comes back --
 * so every live tile has had every sample [0, done) and a pass keeps one first sample.
 * THE CONTRACT: after any sequence of passes and freezes, slot k holds exactly the samples [0, n_k) of its pixels, and its resolved
 * floats and bytes equal, bit for bit, what a UNIFORM accumulation of the same parameters and budget resolves for that tile after
 * n_k samples; the counters summed over all passes equal the sum over slots of the counters of that slot's samples [0, n_k).  With
 * nothing frozen the frame after the budget is the one-shot frame, as before.
 *   - rt_hip_tile_error: the error estimate of every tile from two compact tile-major float buffers as rt_hip_accum_resolve writes
 *     them, d_cur (means of the first n samples) and d_prev (of the first h < n); asynchronous on `stream`, on the device that holds
 *     d_cur; a pure function of its buffers.  fp64 + - * / sqrt in the order written, floats widened exactly, eps = 2^-10:
 *       pixel p of a tile, inside the image and all six channel values finite:
 *         d = (|cur.r - prev.r| + |cur.g - prev.g|) + |cur.b - prev.b|,  l = (cur.r + cur.g) + cur.b,  l = (l > 0) ? l : 0,
 *         e_p = d / sqrt(l + eps);  any other pixel: e_p = +0.0 (outside the image; or NaN / inf, which more samples cannot cure);
 *       tile: v = e[0..64); for m = 32, 16, 8, 4, 2, 1: v[i] = v[i] + v[i + m] for i < m;  E = float(v[0] / valid), valid = the
 *         number of the tile's pixels inside the image.
 *     Half the distance between the means of the two halves of the samples, relative to the pixel's brightness: the measure of
 *     Dammertz et al.'s hierarchical stopping condition, per 8x8 tile.  d_error: one float per slot.
 *   - rt_hip_accum_freeze: slot k stays live iff it is live AND some slot u of the accumulation whose tile lies within Chebyshev
 *     distance `dilate` (0 .. 2 tiles, in the image's tile grid) of slot k's tile has !(E[u] <= threshold) -- a NaN error keeps;
 *     with tile_stride > 1 the tiles that are not in the accumulation do not vote.  Every other live slot freezes at the samples
 *     done so far.  threshold <= 0 freezes nothing.  Runs on `stream` and WAITS on it for *live_count (the next pass's grid needs it).
 *     rt_hip_accum_freeze_mask imposes a host mask instead (h_keep: one byte per slot, 0 = freeze; a frozen slot stays frozen).
 *   - rt_hip_accum_add / _add_host with frozen tiles render the live slots only (the chunks are planned for that many tiles) and
 *     count what they rendered; with no live tile they return RT_HIP_OK, render nothing and the samples done do NOT advance.
 *   - rt_hip_accum_resolve / _read_image divide every slot by its own count once a tile is frozen.
 *   - rt_hip_accum_tile_samples: the sample-count map, one word per slot (a live slot: the samples done); a copy on the null stream.
 *   - rt_hip_accum_run_adaptive: the driver for C hosts, synchronous, on the null stream, from an empty accumulation.  Passes end
 *     at the targets of rt_hip_adapt_schedule: h = max(1, min_samples / 2), then 2h, 4h, ... and the budget.  The first target is
 *     resolved into `prev`; after every later target below the budget: resolve into `cur`, rt_hip_tile_error, rt_hip_accum_freeze,
 *     on_checkpoint(user, samples done, live tiles) (may be NULL; nonzero return: RT_HIP_ECANCELLED), swap; it ends when the budget is
 *     spent or no tile is live.  The last pass is followed by no estimate.  threshold = +inf freezes every tile at the first
 *     checkpoint (2h samples).  h_stats (RT_HIP_NSTATS, may be NULL) += what was rendered; kernel_seconds (may be NULL) = device time
 *     of the passes, resolves, estimates and freezes.
 *     kernel_seconds sums two timers: the passes' own (rt_hip_accum_add_host) and one around every checkpoint's resolve,
 *     estimate and freeze.  With threshold <= 0 no resolve and no estimate is made at all: the passes alone.
 *   - rt_hip_render_adaptive_image: the whole image for C hosts, synchronous: a scene and an accumulation of its own on logical
 *     device `device` of rt_hip_render_image's device map (the HIP device itself without a map), the driver (adapt == NULL: the
 *     defaults), then the row-major frame (h_rgb, h_rgb8: either may be NULL, not both), the count map (h_tile_samples, may be
 *     NULL: ceil(w/8) x ceil(h/8) words, row-major) and the counters (h_stats, overwritten, may be NULL).  params->tile_* are
 *     ignored.  When on_checkpoint cancels, the outputs hold the frame of the samples done and the call returns RT_HIP_ECANCELLED.
 *   - Streams: a freeze rewrites the slot list on ITS stream and a pass reads it on the pass's; like the passes themselves, the
 *     freezes, passes and resolves of one accumulation must be ordered by the caller when their streams differ.  A freeze that
 *     fails on the device after the list was rewritten leaves the accumulation unusable (RT_HIP_ERUNTIME from then on).
 *   - rt_hip_adapt_schedule: the pass targets for a budget (ascending, the last is the budget) into targets[0 .. cap); returns how
 *     many there are (0 for a budget or min_samples below 1).  No device.
 *   - rt_hip_adapt_defaults: min_samples 16, threshold 0.02, dilate 1. */
typedef struct
{
  int32_t min_samples; /* >= 1: the first estimate compares min_samples / 2 with min_samples samples */
  uint32_t dilate;     /* 0 .. 2 tiles */
  double threshold;    /* a tile whose error (and whose neighbours') is <= threshold stops */
} RtHipAdaptParams;
void rt_hip_adapt_defaults(RtHipAdaptParams *params);
int rt_hip_adapt_schedule(int32_t budget, int32_t min_samples, int32_t *targets, int32_t cap);
int rt_hip_tile_error(const float *d_cur, const float *d_prev, int32_t width, int32_t height, uint32_t tile_first, uint32_t tile_stride,
                      uint32_t tile_count, float *d_error, void *stream);
int rt_hip_accum_freeze(RtHipAccum *accum, const float *d_error, double threshold, uint32_t dilate, uint32_t *live_count, void *stream);
int rt_hip_accum_freeze_mask(RtHipAccum *accum, const uint8_t *h_keep, uint32_t *live_count, void *stream);
int rt_hip_accum_tile_samples(const RtHipAccum *accum, uint32_t *h_counts);
uint32_t rt_hip_accum_live_tiles(const RtHipAccum *accum);
int rt_hip_accum_run_adaptive(RtHipAccum *accum, const RtHipAdaptParams *params, uint64_t *h_stats, double *kernel_seconds,
                              int (*on_checkpoint)(void *user, int32_t samples_done, uint32_t live_tiles), void *user);
int rt_hip_render_adaptive_image(const RtHipSphere *spheres, size_t n_spheres, const RtHipMesh *meshes, size_t n_meshes,
                                 const RtHipCamera *camera, const RtHipParams *params, const RtHipAdaptParams *adapt, int device,
                                 float *h_rgb, uint8_t *h_rgb8, uint32_t *h_tile_samples, uint64_t *h_stats, double *kernel_seconds,
                                 int (*on_checkpoint)(void *user, int32_t samples_done, uint32_t live_tiles), void *user);

/* ---- first-hit feature buffers (AOVs): albedo, normal, depth, object id ---------------------------------------------------
 * What a denoiser wants next to the noisy colour (albedo and normal of the first hit, averaged over the same camera samples), and
 * what viewers and compositors want for picking and masks (depth, object id).  A launch uses params->width, height, seed and the
 * tile_* fields; params->samples is S (>= 1); max_depth and integrator are ignored.  For each pixel (x, y) of the launch's tiles and
 * each sample s = 0 .. S-1:
 *   1. the camera ray of beauty sample s: the first two draws r0, r1 of the (seed, y*w + x, s) stream (rt_rng.h),
 *      u = (x + r0) / (w - 1), v = (y + r1) / (h - 1), get_camera_ray -- so S = the frame's spp describes the frame's own samples;
 *   2. the closest hit of intersect() (spheres first, then meshes in array order; strict <, the first index wins a tie): its t;
 *      its OBJECT ID (sphere i: i; a mesh: n_spheres + its index -- rt_hip_scene_create's numbering); its UNIT NORMAL as
 *      trace_path uses it (spheres vec3_normalize(point - centre), triangles calculate_surface_normal; never flipped toward the
 *      viewer); its ALBEDO, the object's color -- on M_CHECKERED objects checkered_texture(color, hit.u, hit.v, 100000) with the
 *      (u, v) trace_path textures with (on meshes: the last passing triangle's) -- not divided by the roulette probability;
 *   3. a sample that hits nothing: albedo = BACKGROUND (10/255 per channel), normal = 0.
 * Per pixel: albedo, normal = the fp64 vec3_add of the samples in ascending order from 0, times 1.0 / S (fp64), rounded to float;
 * hits = how many samples hit; depth = the smallest t of those that hit, as float (+inf: none); object = the id of the sample that
 * gave depth, the lowest s on equal t (0xFFFFFFFF: none).  All of it is fp64 arithmetic in a fixed order: the buffers equal a CPU
 * evaluation of the reference's own code bit for bit.
 *   - rt_hip_render_aov_tiles: asynchronous on `stream`.  d_tiles holds device pointers, each may be NULL but not all; the
 *     buffers are compact tile-major as rt_hip_render_tiles': tile k of the launch owns albedo / normal [k*192, +192) floats and
 *     depth / object / hits [k*64, +64) words; pixels of a tile outside the image read 0 (object 0xFFFFFFFF).  An AOV launch
 *     takes no pending-ray pool, parked-walk workspace, chunk workspace or status word: it has nothing to run out of.
 *   - rt_hip_untile_aov scatters such buffers (those non-NULL in both structs) into row-major images (w*h*3 / w*h words).
 *   - rt_hip_render_aov_image: the whole image, synchronous, on one device -- logical device `device` of rt_hip_render_image's
 *     device map (the HIP device itself without a map) -- into host arrays (h_image: row-major, each may be NULL, not all).
 *   - rt_hip_aov_kernel_name names the form a scene's launches take; rt_hip_aov_kernel_count / _launches list the forms and how
 *     many launches of each this process has made (the AOV kernels are not members of the family of rt_hip_kernel_count). */
typedef struct
{
  float *albedo, *normal, *depth; /* 3, 3, 1 floats per pixel */
  uint32_t *object, *hits;        /* 1 word per pixel */
} RtHipAov;
int rt_hip_render_aov_tiles(const RtHipScene *scene, const RtHipCamera *camera, const RtHipParams *params, const RtHipAov *d_tiles,
                            void *stream);
int rt_hip_untile_aov(const RtHipAov *d_tiles, int32_t width, int32_t height, uint32_t tile_first, uint32_t tile_stride,
                      uint32_t tile_count, const RtHipAov *d_image, void *stream);
int rt_hip_render_aov_image(const RtHipSphere *spheres, size_t n_spheres, const RtHipMesh *meshes, size_t n_meshes,
                            const RtHipCamera *camera, const RtHipParams *params, int device, const RtHipAov *h_image);
const char *rt_hip_aov_kernel_name(const RtHipScene *scene);
int rt_hip_aov_kernel_count(void);
const char *rt_hip_aov_kernel_launches(int index, uint64_t *launches);

/* ---- ray queries: the closest hits of rays the caller chooses --------------------------------------------------------------
 * What the scene scan of the render kernels answers for their own rays, for any rays: picking, line-of-sight and visibility tests,
 * range sensors, collision probes.  A query takes n rays (0 <= n < 2^32).  Ray i comes from params->source:
 *   RT_HIP_RAYS_GIVEN      d_rays holds n x 6 doubles (origin, direction), used as given;
 *   RT_HIP_RAYS_CAMERA_UV  d_rays holds n x 2 doubles (u, v): the ray is get_camera_ray(params->camera, u, v) (raytracer.c:375-384),
 *                          operation for operation, as the render kernels form it from a sample's two draws; u, v may lie outside [0, 1].
 * With RT_HIP_RAYS_NORMALIZE in params->flags the direction is first replaced by vec3_normalize(d) (vector.h:53-58):
 * m = sqrt((x*x + y*y) + z*z), then d * (1.0 / m), fp64, unfused, correctly rounded sqrt and reciprocal.
 * d_t_max (n doubles; NULL: DBL_MAX for every ray) is a per-ray limit that makes the query a visibility test.
 * A ray is INVALID (status 2) if any component of its origin is not finite; or any component of the direction the scan would use is
 * not finite; or | ((dx*dx + dy*dy) + dz*dz) - 1 | > 2^-13 for that direction; or its t_max is NaN.  Every other ray is scanned.
 * The result is that of intersect() (raytracer.c:393-464) with hit->t = DBL_MAX on entry: spheres 0 .. n_spheres-1, then meshes in
 * array order, triangles in order, strict <, the first in scan order wins a tie.  The ray is a HIT (status 1) iff the winner's
 * t < t_max (strict), otherwise a MISS (status 0).  Outputs are structure-of-arrays (RtHipHits; each pointer may be NULL, not all):
 *   field   per ray    hit                                                                         miss / invalid
 *   status  uint32     1                                                                           0 / 2
 *   t       double     the winner's own t (the closest hit's, not what a later, farther primitive    +inf
 *                      left in the reference's Hit.t)
 *   object  uint32     rt_hip_scene_create's id (sphere i: i; a mesh: n_spheres + its index)       0xFFFFFFFF
 *   prim    uint32     triangles: the global index in upload order (through the meshes in array    0xFFFFFFFF
 *                      order), whatever order the hierarchy stores them in; spheres: 0xFFFFFFFF
 *   point   3 double   point_at(ray, t) = o + d*t, unfused                                         0
 *   normal  3 double   as the AOV contract: spheres vec3_normalize(point - centre), triangles       0
 *                      calculate_surface_normal; never flipped
 *   bary    2 double   triangles: the winner's own barycentric (u, v) as intersect_triangle leaves  0
 *                      them, read off as the texture blend of the corners (0, 0), (1, 0), (0, 1): the value
 *                      of rt_hip_selftest_intersect's h_tuv[1..2] plus 0.0 -- equal to it but for a zero,
 *                      which is -0.0 there for some rays through a vertex or along an edge and always
 *                      +0.0 here, as the blend leaves it; spheres: 0
 *   ray     6 double   the ray the scan used, after CAMERA_UV / NORMALIZE (also for misses; invalid rays: as computed)
 * Everything is fp64 in the reference's order: for every valid ray the outputs equal the compiled reference bit for bit.
 * params->origin_radius (>= 0, finite) is a hint for how far from the world origin the rays start.  It takes the place of the
 * camera distance in near_R = 1.5 (origin_radius + reach) + 1 and in everything derived from it (the filter tables); it trades
 * filter tightness against the fallback and does not change a single output bit: a ray that starts beyond near_R is scanned
 * without the filter.  near_R >= 1e15: RT_HIP_EINVAL.
 *   - rt_hip_query_defaults: source GIVEN, flags 0, camera NULL, origin_radius 0.
 *   - rt_hip_query_rays: asynchronous on `stream`, on the scene's device.  d_rays must be 16-byte aligned.  Arguments are checked
 *     before the device is looked for (RT_HIP_EINVAL, then RT_HIP_ENODEV).  n == 0 is RT_HIP_OK and launches nothing.  A query takes
 *     no pool, workspace or status word: it has nothing to run out of.
 *   - rt_hip_query_rays_host: the same from host arrays, synchronous, with a scene and buffers of its own, on logical device
 *     `device` of rt_hip_render_image's device map (the HIP device itself without a map).
 *   - rt_hip_query_kernel_name names the form a scene's queries take; rt_hip_query_kernel_count / _launches list the forms and how
 *     many launches of each this process has made (the query kernels are not members of the family of rt_hip_kernel_count). */
enum
{
  RT_HIP_RAYS_GIVEN = 0,
  RT_HIP_RAYS_CAMERA_UV = 1
};
enum
{
  RT_HIP_RAYS_NORMALIZE = 1u
};
typedef struct
{
  uint32_t source;           /* RT_HIP_RAYS_GIVEN | RT_HIP_RAYS_CAMERA_UV */
  uint32_t flags;            /* RT_HIP_RAYS_NORMALIZE */
  const RtHipCamera *camera; /* host pointer; used with RT_HIP_RAYS_CAMERA_UV */
  double origin_radius;      /* >= 0, finite */
} RtHipQueryParams;
typedef struct
{
  uint32_t *status;
  double *t;
  uint32_t *object, *prim;
  double *point, *normal, *bary, *ray; /* 3, 3, 2, 6 doubles per ray */
} RtHipHits;
void rt_hip_query_defaults(RtHipQueryParams *params);
int rt_hip_query_rays(const RtHipScene *scene, const double *d_rays, const double *d_t_max, uint64_t n, const RtHipQueryParams *params,
                      const RtHipHits *d_hits, void *stream);
int rt_hip_query_rays_host(const RtHipSphere *spheres, size_t n_spheres, const RtHipMesh *meshes, size_t n_meshes, const double *h_rays,
                           const double *h_t_max, uint64_t n, const RtHipQueryParams *params, int device, const RtHipHits *h_hits);
const char *rt_hip_query_kernel_name(const RtHipScene *scene);
int rt_hip_query_kernel_count(void);
const char *rt_hip_query_kernel_launches(int index, uint64_t *launches);

/* ---- radiance queries: trace_path along rays the caller chooses -------------------------------------------------------------
 * What light arrives along a ray: light probes and lightmap baking (rays that start on surfaces), panoramic, fisheye or orthographic
 * views, thin-lens depth of field, resampling of chosen pixels, sensor simulation -- trace_path() (raytracer.c:482-554) with a first
 * ray that no pinhole camera forms.  A call takes n rays (0 <= n < 2^32) and params->samples = S >= 1 samples per ray.
 * Ray i is formed exactly as rt_hip_query_rays forms it (RT_HIP_RAYS_GIVEN, or RT_HIP_RAYS_CAMERA_UV operation for operation, with
 * RT_HIP_RAYS_NORMALIZE the direction through vec3_normalize first) and is INVALID under that contract's rule without its t_max
 * clause: a component of the origin or of the direction is not finite, or | ((dx*dx + dy*dy) + dz*dz) - 1 | > 2^-13.
 * Sample s of a valid ray: the RNG state is that of the stream (seed, index_first + i, s) of rt_rng.h; its first two draws are taken
 * and discarded -- they are render()'s jitter (raytracer.c:203-206), so a sample of a pixel and a sample of a ray with that index
 * see the same draws -- and the sample's value is trace_path(&ray, scene, n, 0) at MAX_DEPTH = params->max_depth with the stream
 * going on from the third draw.
 * The mean, in the order of the static render kernels: S_k (k = 0 .. 3) is the ascending vec3_add, from +0.0, of the samples with
 * s = k (mod 4); total = (S_0 + S_1) + (S_2 + S_3); radiance = total * (1.0 / (double)S).
 * Outputs are structure-of-arrays (RtHipRadiance; each pointer may be NULL, not all):
 *   field     per ray              valid ray                                                         invalid ray
 *   status    uint32               1                                                                 2
 *   radiance  3 double             the mean above                                                    0
 *   samples   3 double per sample  the S sample values, ray-major: sample s of ray i at [i*S + s]    0
 *   paths     uint64               trace_path calls (raytracer.c:484) summed over the ray's samples   0
 *   casts     uint64               scene scans (intersect calls) summed over the ray's samples       0
 *   ray       6 double             the ray used, after CAMERA_UV / NORMALIZE                         as computed
 * d_stats (RT_HIP_NSTATS accumulators, may be NULL) += rays: the sum of paths; casts: the sum of casts; tests: casts x primitives
 * (derived, as everywhere else); samples: valid rays x S.
 * Exactness.  Every decision is the reference's -- hit or miss, the closest index, the roulette, the rejection rounds, the
 * hemisphere flip -- so every draw, and `paths` and `casts` per ray, equal the compiled reference exactly.  The VALUES are those of
 * the render kernels' iteration (Ls += T (.) e; T = T (.) albedo cos), which is the reference's recursion in another association:
 * equal to fp64 rounding (a few 2^-53 per bounce), NOT bit for bit.  Bit-exact are:
 *   (a) radiance is the stated reduction of samples;
 *   (b) results do not depend on how a batch is split: rays [a, b) traced with index_first = a give the bits the same rays get
 *       inside a larger call;
 *   (c) ray equals rt_hip_query_rays' ray for the same input;
 *   (d) the samples values do not depend on S: a sample is a function of (seed, index, s), the ray and the scene.
 * The first scan of a ray in the band that is not unit to 2^-40 drops nothing by a conservative rule, as a query's scan; later
 * bounces keep the rules.  params->origin_radius is rt_hip_query_rays' hint (near_R = 1.5 (origin_radius + reach) + 1, >= 1e15:
 * RT_HIP_EINVAL) and changes no output bit.  params->max_depth: 0 .. 1000000, and <= 32 for scenes with M_REFRACTION materials
 * (RT_HIP_ELIMIT), as rt_hip_render_tiles.  params->integrator must be RT_HIP_TRACE_PATH (cast_ray: RT_HIP_EINVAL).
 *   - rt_hip_trace_defaults: source GIVEN, flags 0, camera NULL, origin_radius 0, samples 1, max_depth 5, seed 0, index_first 0,
 *     integrator RT_HIP_TRACE_PATH.
 *   - rt_hip_trace_rays: asynchronous on `stream`, on the scene's device.  d_rays must be 16-byte aligned; index_first + n <= 2^32.
 *     Arguments are checked before the device is looked for (RT_HIP_EINVAL, then RT_HIP_ENODEV).  n == 0 is RT_HIP_OK and launches
 *     nothing.  The kernels trace M_REFRACTION's two children through the per-device pending-ray pool and report through the
 *     device's status word exactly as the render launches of pt_render_tiles_refr and its siblings do: rt_hip_launch_status tells
 *     of a workgroup that found no slot, and that workgroup's valid rays get NaN radiance and samples (the render's rule).
 *   - rt_hip_trace_rays_host: the same from host arrays, synchronous, with a scene and buffers of its own, on logical device
 *     `device` of rt_hip_render_image's device map; h_stats (may be NULL) += the counters.
 *   - rt_hip_trace_kernel_name names the form a scene's radiance queries take; rt_hip_trace_kernel_count / _launches list the
 *     forms and how many launches of each this process has made (not members of the family of rt_hip_kernel_count). */
typedef struct
{
  uint32_t source;           /* RT_HIP_RAYS_GIVEN | RT_HIP_RAYS_CAMERA_UV, as rt_hip_query_rays */
  uint32_t flags;            /* RT_HIP_RAYS_NORMALIZE */
  const RtHipCamera *camera; /* host pointer; used with RT_HIP_RAYS_CAMERA_UV */
  double origin_radius;      /* as rt_hip_query_rays: a hint, changes no output bit */
  int32_t samples;           /* S >= 1 */
  int32_t max_depth;         /* the reference's MAX_DEPTH */
  uint64_t seed;
  uint32_t index_first;      /* stream index of ray 0; index_first + n <= 2^32 */
  uint32_t integrator;       /* must be RT_HIP_TRACE_PATH */
} RtHipTraceParams;
typedef struct
{
  uint32_t *status;         /* 1 traced, 2 invalid */
  double *radiance;         /* 3 per ray: the mean over the S samples */
  double *samples;          /* 3 per (ray, sample), ray-major: [i*S + s]; optional */
  uint64_t *paths, *casts;  /* per ray, summed over its samples */
  double *ray;              /* 6 per ray: the ray used */
} RtHipRadiance;
void rt_hip_trace_defaults(RtHipTraceParams *params);
int rt_hip_trace_rays(const RtHipScene *scene, const double *d_rays, uint64_t n, const RtHipTraceParams *params,
                      const RtHipRadiance *d_out, uint64_t *d_stats, void *stream);
int rt_hip_trace_rays_host(const RtHipSphere *spheres, size_t n_spheres, const RtHipMesh *meshes, size_t n_meshes, const double *h_rays,
                           uint64_t n, const RtHipTraceParams *params, int device, const RtHipRadiance *h_out, uint64_t *h_stats);
const char *rt_hip_trace_kernel_name(const RtHipScene *scene);
int rt_hip_trace_kernel_count(void);
const char *rt_hip_trace_kernel_launches(int index, uint64_t *launches);

/* ---- thin-lens camera: depth of field from generated lens rays ------------------------------------------------------------------
 * A frame with depth of field is made of three pieces: a kernel that writes the LENS RAYS of one sample pass, the radiance query
 * above (rt_hip_trace_rays, called as it stands: no render, accumulation or pixel-list kernel knows of a lens), and a kernel that
 * folds the pass into a per-pixel sum, with a resolve.  What is new is a pure function of its arguments and is stated here operation
 * for operation; everything about paths is rt_hip_trace_rays' contract.
 *
 * THE LENS RAY of pixel p = y*width + x and sample s, NP = width*height, under a camera, a seed and an RtHipLens.  fp64 + - * / sqrt,
 * unfused, in the order written; vec3_* are vector.h's (vec3_normalize(a) = a * (1.0 / sqrt((a.x*a.x + a.y*a.y) + a.z*a.z))):
 *   stream index   k = s*NP + p.  The frame lives in the ray-index space of rt_hip_trace_rays, one sample per ray: (s + 1)*NP <= 2^32.
 *   jitter         r0, r1 = the first two draws of the stream (seed, k, 0) of rt_rng.h; u = ((double)x + r0) / ((double)width - 1.0),
 *                  v = ((double)y + r1) / ((double)height - 1.0) (raytracer.c:203-204).  These are the two draws rt_hip_trace_rays
 *                  discards before the path starts: jitter and path share one stream without overlap.
 *   direction      d = position - (lower_left_corner + (horizontal*u + vertical*v)), get_camera_ray's order (raytracer.c:377-381),
 *                  NOT normalised.  For a camera made by init_camera d = forward + (0.5 - u) horizontal + (0.5 - v) vertical: its
 *                  forward component is 1, so position + d*f lies on the plane at distance f in front of the camera.
 *   focus point    F = position + d*focus_distance.
 *   lens axes      ax = vec3_normalize(horizontal), ay = vec3_normalize(vertical), made once on the host.
 *   lens point     from a second stream, so that the path's draws do not move: state rt_rng_seed(rt_mix64(seed ^ 0x6C656E73), k, 0).
 *                  A round draws r1 then r2, a = 2.0*r1 - 1.0, b = 2.0*r2 - 1.0, and is accepted iff a*a + b*b < 1.0; the first
 *                  accepted round of at most 32 gives (a, b); if none accepts, a = b = 0.0 (the centre of the lens).
 *                  L = position + (ax*(a*R) + ay*(b*R)) with R = aperture_radius.
 *   ray            origin L, direction vec3_normalize(F - L).
 * Where the origins lie: a*a + b*b < 1, so with horizontal and vertical orthogonal |L - position| <= R to rounding (the offset
 * ax*(a*R) + ay*(b*R) itself is within R (1 + 2^-50)); a sheared camera's lens is the parallelogram's ellipse, within
 * R sqrt(1 + |ax . ay|) of the position.
 * aperture_radius == 0 runs the same formula -- L = position + (ax*0 + ay*0), the direction through F -- and is NOT promised to
 * equal the pinhole ray of get_camera_ray bit for bit (F - L is d*focus_distance after two more roundings).
 * A camera whose horizontal, vertical or lower_left_corner is not finite (or overflows on the way), horizontal or vertical of
 * length 0, or F == L give a ray that rt_hip_trace_rays calls INVALID (status 2); rt_hip_lens_rays writes it as computed.
 *
 * THE FRAME (rt_hip_render_lens): of params, width, height, samples = S, max_depth and seed are used; integrator must be
 * RT_HIP_TRACE_PATH; the tile fields must describe the whole frame (tile_first 0, tile_stride 0 or 1, tile_count 0 or all tiles).
 * sum is zeroed to +0.0; for s = 0 .. S-1 and each slice of at most slice_pixels pixels in ascending order: the slice's lens rays;
 * rt_hip_trace_rays' own launch with samples = 1, index_first = s*NP + the slice's first pixel, RT_HIP_RAYS_GIVEN and origin_radius
 * = |position| + aperture_radius (a hint: it changes no bit); sum[p] = vec3_add(sum[p], radiance[p]) -- so in ascending s --, and a ray
 * of status 2 makes its pixel's sum a quiet NaN in all three channels.  Then mean = sum * (1.0 / (double)S), rgb = (float)mean and rgb8 =
 * the render epilogue's gamma-5 tonemap of mean (the device function rt_hip_accum_resolve's kernels call), row-major, not tiled.
 * Everything goes on `stream` with no host wait between passes; d_stats (may be NULL) accumulates rt_hip_trace_rays' counters.
 * CONTRACT:
 *   (a) the rays equal the statement above bit for bit;
 *   (b) sample s of pixel p is what rt_hip_trace_rays returns for that ray at index_first + i = s*NP + p, samples = 1: `paths` and
 *       `casts` equal the compiled reference's per ray, and the values are inside that contract's bar;
 *   (c) sum, rgb and rgb8 are the stated reductions of those samples, bit for bit;
 *   (d) no output bit depends on slice_pixels;
 *   (e) scenes with M_REFRACTION report through the device's status word exactly as rt_hip_trace_rays says.
 *   - rt_hip_lens_defaults: aperture_radius 0, focus_distance 1, flags 0.
 *   - rt_hip_lens_rays: the generator alone: rays of pixels [pixel_first, pixel_first + n) of sample `sample` into d_rays (n x 6
 *     doubles, 16-byte aligned, as rt_hip_trace_rays takes them); pixel_first + n <= NP; asynchronous on `stream`, on the device
 *     that holds d_rays.  n == 0 is RT_HIP_OK and launches nothing.
 *   - rt_hip_lens_workspace_bytes: the d_workspace of rt_hip_render_lens (a slice's rays, status words and radiance, and the frame's
 *     sums, 24 bytes a pixel, whether or not d_sum is given); 0 for a size out of range or slice_pixels == 0.
 *   - rt_hip_render_lens: d_sum (3 doubles a pixel) may be NULL: the sums then live in the workspace; d_rgb (3 floats a pixel) and
 *     d_rgb8 (3 bytes) may each be NULL, but one of the three outputs is required.  slice_pixels above NP means NP.
 *   - rt_hip_lens_resolve: the resolve alone, for a caller that keeps d_sum: mean = sum * (1.0 / (double)samples) of width x height
 *     pixels into d_rgb and d_rgb8 (either may be NULL, not both) by the rule above; total: any bits in sum have a result (a NaN or
 *     negative mean reads byte 255 or 0 as the tonemap has it).  Asynchronous on `stream`, on the device that holds d_sum.
 *   - rt_hip_render_lens_image: the host form, synchronous, with a scene and buffers of its own on logical device `device` of
 *     rt_hip_render_image's device map; h_rgb, h_rgb8: either may be NULL, not both; h_stats (may be NULL) is overwritten; it checks
 *     the device's status word (rt_hip_launch_status) and returns its error.
 * Refusals, each before the first launch and with the outputs untouched, arguments before the device is looked for.  RT_HIP_EINVAL:
 * aperture_radius negative, NaN or infinite; focus_distance not finite or <= 0; lens flags or reserved not 0; width or height < 2 (or
 * above 2^20); samples < 1; samples * NP > 2^32; slice_pixels == 0; RT_HIP_CAST_RAY; tile fields of a part of the frame; max_depth
 * outside 0 .. 1000000; a NULL required pointer; a d_workspace or d_rays that is not 16-byte aligned, a d_sum that is not 8-byte
 * aligned; a camera position that is not finite; near_R >= 1e15 (rt_hip_trace_rays' rule).  RT_HIP_ELIMIT: max_depth above 32 with an
 * M_REFRACTION material, as rt_hip_trace_rays. */
typedef struct
{
  double aperture_radius; /* R >= 0, finite; 0: every ray starts at the camera position */
  double focus_distance;  /* f > 0, finite: the plane at this distance in front of the camera is sharp */
  uint32_t flags;         /* must be 0 */
  uint32_t reserved;      /* must be 0 */
} RtHipLens;
void rt_hip_lens_defaults(RtHipLens *lens);
int rt_hip_lens_rays(const RtHipCamera *camera, const RtHipLens *lens, int32_t width, int32_t height, uint64_t seed, uint32_t sample,
                     uint32_t pixel_first, uint32_t n, double *d_rays, void *stream);
size_t rt_hip_lens_workspace_bytes(int32_t width, int32_t height, uint32_t slice_pixels);
int rt_hip_render_lens(const RtHipScene *scene, const RtHipCamera *camera, const RtHipLens *lens, const RtHipParams *params,
                       uint32_t slice_pixels, void *d_workspace, double *d_sum, float *d_rgb, uint8_t *d_rgb8, uint64_t *d_stats, void *stream);
int rt_hip_lens_resolve(const double *d_sum, int32_t width, int32_t height, int32_t samples, float *d_rgb, uint8_t *d_rgb8, void *stream);
int rt_hip_render_lens_image(const RtHipSphere *spheres, size_t n_spheres, const RtHipMesh *meshes, size_t n_meshes, const RtHipCamera *camera,
                             const RtHipLens *lens, const RtHipParams *params, int device, float *h_rgb, uint8_t *h_rgb8, uint64_t *h_stats);

/* ---- light probes: SH9 radiance and irradiance baked from generated probe rays -----------------------------------------------------
 * A bake is made of three pieces, as a lens frame is: a kernel that writes the PROBE RAYS of a slice of ray indices, the radiance
 * query above (rt_hip_trace_rays, called as it stands) and a kernel that folds the slice's samples into per-probe sums, with a
 * resolve.  What is new is a pure function of its arguments and is stated here operation for operation; everything about paths is
 * rt_hip_trace_rays' contract.  The reference has no probe code: its random_on_unit_sphere and random_on_hemisphere are restated.
 *
 * RAY INDEX SPACE.  N probes, S = params->samples samples a probe; the ray of (probe i, sample s) has index k = i*S + s (probe-major: a
 * slice of consecutive k keeps the device full even for few probes); N*S <= 2^32.
 *
 * THE PROBE RAY of index k under a seed.  fp64 + - * / sqrt, unfused, in the order written:
 *   stream         state rt_rng_seed(rt_mix64(seed ^ 0x70726F62), k, 0) of rt_rng.h: a stream of its own, as the lens has one.  The
 *                  path's stream (seed, k, 0) is untouched, and the two draws rt_hip_trace_rays discards stay unused.
 *   a round        random_on_unit_sphere's (raytracer.c:231-243): draws r1, r2, r3; x = r1*2.0 + -1.0, y and z likewise;
 *                  q = (x*x + y*y) + z*z; accepted iff q <= 1.0 && q >= 2^-20.  The first accepted round of at most 32 gives
 *                  d = (x, y, z) * (1.0 / sqrt(q)); if none accepts, d = (0, 0, 1) (probability about 5e-11 a ray).
 *   RT_HIP_PROBE_SPHERE      origin = the probe's position (3 doubles), direction d.
 *   RT_HIP_PROBE_HEMISPHERE  needs normals (3 doubles a probe, used as given: not normalised) and bias >= 0:
 *                  c = (d.x*n.x + d.y*n.y) + d.z*n.z; if c < 0 then d = d * -1.0 (random_on_hemisphere, :245-253); origin =
 *                  position + n*bias.
 * A position or normal that is not finite gives a ray that rt_hip_trace_rays calls INVALID (status 2); it is written as computed.
 *
 * THE FOLD.  With the ray's stored direction (x, y, z) and its sample `radiance` (3 doubles), for every basis j and channel c, over
 * the probe's rays in ascending k from +0.0: sum = sum + (radiance[c] * w_j), the product rounded before the add.  A ray of status 2
 * makes all of its probe's sums NaN (isnan; sign and payload unspecified).
 *   SPHERE, 9 bases (real spherical harmonics to l = 2):  w0 = Y0, w1 = Y1*y, w2 = Y1*z, w3 = Y1*x, w4 = Y2A*(x*y), w5 = Y2A*(y*z),
 *     w6 = Y2B*(3.0*(z*z) - 1.0), w7 = Y2A*(x*z), w8 = Y2C*(x*x - y*y), with Y0 = 0.28209479177387814, Y1 = 0.4886025119029199,
 *     Y2A = 1.0925484305920792, Y2B = 0.31539156525252005, Y2C = 0.5462742152960396.
 *   HEMISPHERE, 1 basis:  c = (x*n.x + y*n.y) + z*n.z; w0 = c > 0 ? c : 0.0.
 * THE RESOLVE.  coeff = (sum * (1.0 / (double)S)) * K; K = 12.566370614359172 (4 pi) for SPHERE: the SH9 radiance coefficients,
 * N x 9 x 3 doubles [probe][basis][channel]; K = 6.283185307179586 (2 pi) for HEMISPHERE: the irradiance E, N x 1 x 3.  The float
 * copy is (float)coeff.
 * IRRADIANCE FROM SH9 (rt_hip_probe_irradiance): m entries of a probe index (uint32) and a normal n (3 doubles, used as given);
 * E_c = the ascending sum from +0.0 over j = 0 .. 8 of (A_j * coeff[i][j][c]) * w_j(n), w_j as above, A_0 = 3.141592653589793,
 * A_1..3 = 2.0943951023931953, A_4..8 = 0.7853981633974483 (the cosine lobe's band factors).  A probe index >= N gives a quiet NaN:
 * the function is total.
 *
 * THE BAKE (rt_hip_bake_probes): the sums are zeroed to +0.0 and the probes' status to 1; the ray indices are walked in ascending
 * slices of at most slice_rays rays (above N*S means N*S): the slice's rays; rt_hip_trace_rays' own launch with samples = 1,
 * index_first = the slice's first k, RT_HIP_RAYS_GIVEN and origin_radius = params->origin_radius (the caller's hint: every origin
 * lies within it of the world's origin; it changes no bit); the fold.  Then the resolve.  Everything goes on `stream` with no host
 * wait between slices; d_stats (may be NULL) accumulates rt_hip_trace_rays' counters.
 * CONTRACT:
 *   (a) the rays equal the statement above bit for bit;
 *   (b) sample s of probe i is what rt_hip_trace_rays returns for that ray at index_first + j = i*S + s, samples = 1: `paths` and
 *       `casts` equal the compiled reference's per ray, and the values are inside that contract's bar;
 *   (c) sums, coefficients and their float copy are the stated reductions of those samples, bit for bit;
 *   (d) one thread adds a sum in ascending k across slices: no output bit depends on slice_rays;
 *   (e) scenes with M_REFRACTION report through the device's status word exactly as rt_hip_trace_rays says.
 *   - rt_hip_probe_defaults: mode SPHERE, flags 0, samples 64, max_depth 5, seed 0, bias 0, origin_radius 0, reserved 0.
 *   - rt_hip_probe_rays: the generator alone: rays [k_first, k_first + n) into d_rays (n x 6 doubles, 16-byte aligned, as
 *     rt_hip_trace_rays takes them); k_first + n <= N*S; max_depth and origin_radius are not used; asynchronous on `stream`, on the
 *     device that holds d_rays.  n == 0 is RT_HIP_OK and launches nothing.
 *   - rt_hip_probe_workspace_bytes: the d_workspace of rt_hip_bake_probes for slices of slice_rays rays (a slice's rays, status
 *     words and radiance, 76 bytes a ray, and the sums, 24 bytes a basis and probe, whether or not d_sum is given).  A caller whose
 *     slice_rays exceeds N*S may size it with N*S.  0 for an unknown mode or slice_rays == 0.
 *   - rt_hip_bake_probes: d_positions (and d_normals for HEMISPHERE) hold 3 doubles a probe.  d_sum (N x bases x 3 doubles) may be
 *     NULL: the sums then live in the workspace; d_coeff (the same shape) is required; d_coeff_f (floats) and d_status (a uint32 a
 *     probe: 1, or 2 if any of its rays was invalid) may be NULL.
 *   - rt_hip_probe_resolve: the resolve alone, for a caller that keeps d_sum; d_coeff_f may be NULL.  Asynchronous on `stream`, on
 *     the device that holds d_sum.
 *   - rt_hip_probe_irradiance: d_coeff holds n_probes x 9 x 3 doubles; d_irradiance gets 3 doubles an entry.  m == 0 is RT_HIP_OK.
 *   - rt_hip_bake_probes_host: the host form, synchronous, with a scene and buffers of its own on logical device `device` of
 *     rt_hip_render_image's device map; h_coeff is required, h_coeff_f and h_status may be NULL; h_stats (may be NULL) is
 *     overwritten; it checks the device's status word (rt_hip_launch_status) and returns its error.
 * Refusals, each before the first launch and with the outputs untouched, arguments before the device is looked for.  RT_HIP_EINVAL:
 * an unknown mode; flags or reserved not 0; samples < 1; n_probes * samples > 2^32; slice_rays == 0; bias or origin_radius negative
 * or not finite; HEMISPHERE without normals; max_depth outside 0 .. 1000000; a d_workspace or d_rays that is not 16-byte aligned; a
 * NULL required pointer; near_R >= 1e15 (rt_hip_trace_rays' rule).  RT_HIP_ELIMIT: max_depth above 32 with an M_REFRACTION material,
 * as rt_hip_trace_rays.  n_probes == 0 with good params is RT_HIP_OK and launches nothing. */
enum
{
  RT_HIP_PROBE_SPHERE = 0,
  RT_HIP_PROBE_HEMISPHERE = 1
};
typedef struct
{
  uint32_t mode;        /* RT_HIP_PROBE_SPHERE | RT_HIP_PROBE_HEMISPHERE */
  uint32_t flags;       /* must be 0 */
  int32_t samples;      /* S >= 1 rays a probe */
  int32_t max_depth;    /* the reference's MAX_DEPTH */
  uint64_t seed;
  double bias;          /* >= 0, finite: a hemisphere probe's rays start at position + normal*bias */
  double origin_radius; /* as rt_hip_trace_rays: a hint, changes no output bit */
  uint64_t reserved;    /* must be 0 */
} RtHipProbeParams;
void rt_hip_probe_defaults(RtHipProbeParams *params);
int rt_hip_probe_rays(const double *d_positions, const double *d_normals, uint64_t n_probes, const RtHipProbeParams *params, uint64_t k_first,
                      uint64_t n, double *d_rays, void *stream);
size_t rt_hip_probe_workspace_bytes(uint64_t n_probes, uint32_t mode, uint32_t slice_rays);
int rt_hip_bake_probes(const RtHipScene *scene, const double *d_positions, const double *d_normals, uint64_t n_probes,
                       const RtHipProbeParams *params, uint32_t slice_rays, void *d_workspace, double *d_sum, double *d_coeff, float *d_coeff_f,
                       uint32_t *d_status, uint64_t *d_stats, void *stream);
int rt_hip_probe_resolve(const double *d_sum, uint64_t n_probes, uint32_t mode, int32_t samples, double *d_coeff, float *d_coeff_f, void *stream);
int rt_hip_probe_irradiance(const double *d_coeff, uint64_t n_probes, const uint32_t *d_index, const double *d_normals, uint64_t m,
                            double *d_irradiance, void *stream);
int rt_hip_bake_probes_host(const RtHipSphere *spheres, size_t n_spheres, const RtHipMesh *meshes, size_t n_meshes, const double *h_positions,
                            const double *h_normals, uint64_t n_probes, const RtHipProbeParams *params, int device, double *h_coeff,
                            float *h_coeff_f, uint32_t *h_status, uint64_t *h_stats);

/* ---- probe grids: shade entries from a regular grid of baked SH9 probes ------------------------------------------------------------
 * What light reaches a surface point, given the probes around it: a regular GRID of sphere probes, a kernel that SHADES entries (a
 * point and a normal each: the first hits of a frame's pixels, lightmap texels, a moving object's vertices) from the grid's baked
 * coefficients, and the PROBE-LIT PREVIEW of a frame made of a ray query, the albedo of the first-hit buffers and that kernel.  The
 * ray, radiance and first-hit queries are called as they stand; what is new is a pure function of its arguments, stated here.
 *
 * THE GRID (RtHipProbeGrid).  count[0] x count[1] x count[2] = n probes; probe (ix, iy, iz) has index i = (iz*count[1] + iy)*count[0]
 * + ix and on axis a the position origin[a] + (double)i_a * step[a], the product rounded before the add (fp64, unfused).
 *   - rt_hip_probe_grid_defaults: struct_size = sizeof(RtHipProbeGrid), flags 0, origin 0, step 1, count 1, miss_color
 *     (float)(10.0/255.0) in each channel (the reference's background), reserved 0.
 *   - rt_hip_probe_grid_positions: d_positions gets n x 3 doubles, one thread a probe; they feed rt_hip_bake_probes in
 *     RT_HIP_PROBE_SPHERE mode unchanged.  Asynchronous on `stream`, on the device that holds d_positions.
 *   - rt_hip_bake_probe_grid: rt_hip_probe_grid_positions into the workspace, then rt_hip_bake_probes at them, and nothing else:
 *     params->mode must be RT_HIP_PROBE_SPHERE; d_coeff (n x 9 x 3 doubles) is required, d_coeff_f, d_status and d_stats may be NULL;
 *     the sums live in the workspace.  rt_hip_probe_grid_workspace_bytes = rt_hip_probe_workspace_bytes(n, SPHERE, slice_rays) plus
 *     the positions (24 bytes a probe, after the bake's part); 0 for a grid any call would refuse or slice_rays == 0.
 *
 * THE SHADE (rt_hip_probe_shade): m entries, m < 2^32.  d_points and d_normals hold 3 doubles an entry (the layout of RtHipHits.point
 * and .normal: a ray query's output feeds it directly); d_status (may be NULL) the query's status words; d_albedo (may be NULL) 3
 * floats an entry, a row-major AOV albedo image as it stands; d_add (may be NULL) 3 floats an entry, e.g. the emission of what was
 * hit; d_irradiance (3 doubles an entry) and d_color (3 floats an entry) may each be NULL, not both.  Asynchronous on `stream`, on
 * the device that holds d_points.
 * CONTRACT.  All arithmetic is fp64 + - * / sqrt, unfused, in the order written; A_j, w_j(n) and the quiet NaN are those of
 * rt_hip_probe_irradiance above.
 *   1. Class of an entry.  MISS: d_status is given and the word is not 1.  INVALID: not a miss, and any component of its point or
 *      normal is not finite.  Otherwise VALID.
 *   2. Cell.  For each axis a with N = count[a]: g = (p_a - origin[a]) / step[a]; g = g > 0.0 ? g : 0.0; top = (double)(N - 1);
 *      g = g < top ? g : top; i0 = (uint32_t)g (truncates); if N >= 2 && i0 > N - 2 then i0 = N - 2; f = g - (double)i0;
 *      i1 = N >= 2 ? i0 + 1 : 0; w_a[0] = 1.0 - f, w_a[1] = f.  (N == 1: f = 0, w = (1, 0).)
 *   3. Corners.  For c = 0 .. 7 with bx = c & 1, by = (c >> 1) & 1, bz = c >> 2: the probe is (i_x[bx], i_y[by], i_z[bz]);
 *      tri = (w_x[bx] * w_y[by]) * w_z[bz].  Without RT_HIP_GRID_FACING w_c = tri.  With it: v = the corner's position (the grid's
 *      formula) - p; q = (v.x*v.x + v.y*v.y) + v.z*v.z; cs = q > 0.0 ? ((v.x*n.x + v.y*n.y) + v.z*n.z) * (1.0 / sqrt(q)) : 1.0;
 *      s = (cs + 1.0) * 0.5; face = s*s + 0.2; w_c = tri * face.  The normal is used as given, not normalised.
 *   4. Blend.  Over c ascending, from +0.0; a corner with w_c == 0.0 (either sign) is skipped and its coefficients do not enter: a
 *      NaN probe outside the support cannot poison an entry; a NaN weight does not skip.  B[j][ch] = B[j][ch] + (w_c *
 *      coeff[i_c][j][ch]); W = W + w_c.
 *   5. Evaluate.  E_ch = the ascending sum from +0.0 over j = 0 .. 8 of (A_j * B[j][ch]) * w_j(n); E_ch = E_ch / W;
 *      E_ch = E_ch < 0.0 ? 0.0 : E_ch (clamps SH ringing; a NaN stays NaN).
 *   6. A VALID entry: irradiance = E; color_ch = (float)((((double)albedo_ch * E_ch) * 0.3183098861837907) + (double)add_ch); an absent
 *      albedo counts as 1.0f, an absent add as +0.0 (the term is added all the same).
 *   7. MISS: irradiance +0.0, color_ch = (float)((double)miss_color[ch] + (double)add_ch).  INVALID: a quiet NaN in every output, sign
 *      and payload unspecified.
 * The function is TOTAL: any bytes in d_coeff, any finite point and any normal give a defined result, and no index leaves [0, n).
 * The kernel reads a wave's coefficients through wave-uniform loads where the wave's valid entries share a cell and per lane where
 * they do not: the same operations in the same order, the same bits.
 *
 * THE PREVIEW (rt_hip_probe_preview), width, height >= 2, all on `stream` with no host wait: the pixel centres u = ((double)x + 0.5)
 * / ((double)width - 1.0), v = ((double)y + 0.5) / ((double)height - 1.0), pixel p = y*width + x; rt_hip_query_rays' launch with
 * RT_HIP_RAYS_CAMERA_UV at them for status, point, normal and object; rt_hip_render_aov_tiles and rt_hip_untile_aov for the albedo
 * at aov_samples samples under `seed` (the whole frame); add = (float)emission[object], read from the scene's own material records
 * on the device (spheres, then meshes: rt_hip_scene_create's numbering; nothing is uploaded; +0.0f for a miss); the shade; rgb8 = the render epilogue's gamma-5 tonemap of
 * (double)rgb (the device function rt_hip_accum_resolve's kernels call).  d_rgb (3 floats a pixel, row-major) is required, d_rgb8
 * may be NULL.  Bit for bit the composition of those calls; no output bit depends on anything else.
 *   - rt_hip_probe_preview_workspace_bytes: the d_workspace (16-byte aligned) of a width x height preview of `scene`; 0 for a size
 *     out of range.
 *   - rt_hip_probe_preview_image: the host form, synchronous, with a scene and buffers of its own on logical device `device` of
 *     rt_hip_render_image's device map: it bakes the grid (rt_hip_bake_probe_grid under probe_params), runs the preview with
 *     seed = probe_params->seed and reads back h_rgb, h_rgb8 (either may be NULL, not both) and h_coeff (may be NULL); h_stats (may
 *     be NULL) is overwritten with the bake's counters; it checks the device's status word and returns its error.
 *   - rt_hip_probe_preview_scene_image: the same from a scene the caller holds, on that scene's device: for a host that has asked
 *     the scene something first (its bounds, to place the grid) and would otherwise set the scene up twice.
 * Refusals, each before any launch, arguments before a device is looked for.  RT_HIP_EINVAL: a struct_size below the struct's;
 * unknown flags or a non-zero reserved; a step that is not finite or not positive; an origin that is not finite; a count of 0 or a
 * product above 2^24; a miss_color that is not finite; a NULL required pointer, or both outputs NULL; m >= 2^32; for the bake and
 * the preview what rt_hip_bake_probes, rt_hip_query_rays and rt_hip_render_aov_tiles refuse.  m == 0 is RT_HIP_OK and launches
 * nothing. */
enum
{
  RT_HIP_GRID_FACING = 1u
};
typedef struct
{
  uint32_t struct_size; /* set by rt_hip_probe_grid_defaults */
  uint32_t flags;       /* RT_HIP_GRID_FACING or 0 */
  double origin[3];     /* position of probe (0,0,0) */
  double step[3];       /* finite, > 0 */
  uint32_t count[3];    /* each >= 1; count[0]*count[1]*count[2] <= 2^24 */
  float miss_color[3];  /* colour of an entry that is a miss; default (float)(10.0/255.0) x 3 */
  uint32_t reserved;    /* 0 */
} RtHipProbeGrid;
void rt_hip_probe_grid_defaults(RtHipProbeGrid *grid);
int rt_hip_probe_grid_positions(const RtHipProbeGrid *grid, double *d_positions, void *stream);
size_t rt_hip_probe_grid_workspace_bytes(const RtHipProbeGrid *grid, uint32_t slice_rays);
int rt_hip_bake_probe_grid(const RtHipScene *scene, const RtHipProbeGrid *grid, const RtHipProbeParams *params, uint32_t slice_rays,
                           void *d_workspace, double *d_coeff, float *d_coeff_f, uint32_t *d_status, uint64_t *d_stats, void *stream);
int rt_hip_probe_shade(const RtHipProbeGrid *grid, const double *d_coeff, const double *d_points, const double *d_normals,
                       const uint32_t *d_status, const float *d_albedo, const float *d_add, uint64_t m, double *d_irradiance, float *d_color,
                       void *stream);
size_t rt_hip_probe_preview_workspace_bytes(const RtHipScene *scene, int32_t width, int32_t height);
int rt_hip_probe_preview(const RtHipScene *scene, const RtHipCamera *camera, const RtHipProbeGrid *grid, const double *d_coeff, int32_t width,
                         int32_t height, int32_t aov_samples, uint64_t seed, void *d_workspace, float *d_rgb, uint8_t *d_rgb8, void *stream);
int rt_hip_probe_preview_image(const RtHipSphere *spheres, size_t n_spheres, const RtHipMesh *meshes, size_t n_meshes, const RtHipCamera *camera,
                               const RtHipProbeGrid *grid, const RtHipProbeParams *probe_params, int32_t width, int32_t height,
                               int32_t aov_samples, int device, float *h_rgb, uint8_t *h_rgb8, double *h_coeff, uint64_t *h_stats);
int rt_hip_probe_preview_scene_image(const RtHipScene *scene, const RtHipCamera *camera, const RtHipProbeGrid *grid,
                                     const RtHipProbeParams *probe_params, int32_t width, int32_t height, int32_t aov_samples, float *h_rgb,
                                     uint8_t *h_rgb8, double *h_coeff, uint64_t *h_stats);

/* ---- probe visibility: baked depth moments keep a probe behind a wall from lighting the wall's other side ---------------------------
 * RT_HIP_GRID_FACING is a weight, not a visibility test.  This is the usual remedy of irradiance volumes: every probe keeps the mean
 * and the mean square of the distance to the nearest surface in an R x R octahedral MAP of directions, baked from the very rays of
 * its radiance bake by the ray query that exists (query_launch, untouched), and the shade weighs every corner by the Chebyshev bound
 * of the chance that the probe sees the shaded point.  What is new is a pure function of its arguments, stated here.  All arithmetic
 * is fp64 + - * / sqrt, unfused, in the order written; |x| clears the sign bit; sgn(v) = v >= 0.0 ? 1.0 : -1.0.
 *
 * THE PARAMETERS (RtHipProbeVis): res = R (2 .. 32), sharp (0 .. 8), d_max (finite, > 0), bias (finite, >= 0), floor (finite, in
 * (0, 1]); flags and reserved 0.
 *   - rt_hip_probe_vis_defaults(vis, grid): struct_size = sizeof(RtHipProbeVis), flags 0, res 8, sharp 5, with the grid's step
 *     (sx, sy, sz): d_max = 1.5 * sqrt((sx*sx + sy*sy) + sz*sz), bias = 0.125 * min(sx, sy, sz), floor = 2^-6, reserved 0.  A NULL
 *     grid counts as step (1, 1, 1).
 *
 * THE MAP.  Texel (tx, ty), 0 <= tx, ty < R, has index tx + R*ty.  Its CENTRE DIRECTION e: a = (((double)tx + 0.5) / (double)R) * 2.0
 * - 1.0, b likewise from ty; z = (1.0 - |a|) - |b|; if z < 0.0 then (x, y) = ((1.0 - |b|) * sgn(a), (1.0 - |a|) * sgn(b)), else
 * (x, y) = (a, b); e = (x, y, z) * (1.0 / sqrt((x*x + y*y) + z*z)).
 * THE LOOKUP of a probe's map at a direction v (not normalised, not zero):
 *   1. s = (|v.x| + |v.y|) + |v.z|; a = v.x / s; b = v.y / s; if v.z < 0.0 then (a, b) = ((1.0 - |b|) * sgn(a), (1.0 - |a|) * sgn(b)),
 *      both from the unfolded a and b.
 *   2. Per axis, with a (tx) and b (ty): u = (a*0.5 + 0.5) * (double)R - 0.5; u = u >= -0.5 ? u : -0.5 (a NaN reads from -0.5: the
 *      function is total); top = (double)R - 0.5; u = u <= top ? u : top; i0 = floor(u), in -1 .. R-1; f = u - (double)i0; i1 = i0 + 1.
 *   3. A texel (i, j) outside the map is continued across its edge, in this order: if i is out of 0 .. R-1 then i is clamped into it
 *      and j = R-1-j; then if j is out of range then j is clamped and i = R-1-i.  So (-1, j) reads (0, R-1-j), (-1, -1) reads
 *      (R-1, R-1).  Each of the four texels is continued on its own.
 *   4. gx = 1.0 - fx, gy = 1.0 - fy; w00 = gx*gy, w10 = fx*gy, w01 = gx*fy, w11 = fx*fy; with m_ab the value of texel (i_a, j_b):
 *      value = ((w00*m00 + w10*m10) + w01*m01) + w11*m11, for mean and for mean2 alike.
 *
 * THE DEPTH FOLD.  Sums W, M1, M2 per (probe, texel), over the probe's rays in ascending k (the ray index space and the rays of
 * "light probes" above) from +0.0.  For a ray of stored direction d, status word st and distance t from the ray query, and the texel's
 * e: c = (d.x*e.x + d.y*e.y) + d.z*e.z; c = c > 0.0 ? c : 0.0; w = c, then w = w*w `sharp` times (the lobe c^(2^sharp));
 * dist = st == 1 ? (t < d_max ? t : d_max) : d_max; W = W + w; M1 = M1 + w*dist; M2 = M2 + w*(dist*dist).  A ray of status 2 makes
 * all sums of its probe NaN and the probe's status word 2.  One thread owns a (probe, texel) and carries its sums across slices:
 * no bit depends on slice_rays.
 * THE DEPTH RESOLVE.  mean = W > 0.0 ? M1 / W : d_max; mean2 = W > 0.0 ? M2 / W : d_max*d_max; a NaN W (an invalid probe) gives NaN
 * for both.  d_moments: N x R*R x 2 doubles [probe][texel][mean, mean2].
 *
 * THE BAKE (rt_hip_bake_probe_depth), params->mode RT_HIP_PROBE_SPHERE: the sums are zeroed and the probes' status set to 1; the
 * ray indices are walked in ascending slices of at most slice_rays: the slice's probe rays (rt_hip_probe_rays' kernel as it stands:
 * under the same RtHipProbeParams the rays of rt_hip_bake_probes, bit for bit), rt_hip_query_rays' own launch for status and t
 * (RT_HIP_RAYS_GIVEN, no t_max, origin_radius = params->origin_radius), the fold; then the resolve.  All on `stream`, no host wait.
 * params->max_depth is checked as rt_hip_bake_probes checks it and not used.
 *   - rt_hip_probe_depth_workspace_bytes: the d_workspace for slices of slice_rays rays (60 bytes a ray, and the sums, 24 bytes a
 *     texel and probe); 0 for res out of range, slice_rays == 0 or n_probes * res * res > 2^28.
 *   - rt_hip_bake_probe_depth: d_positions 3 doubles a probe; d_moments required; d_status (a uint32 a probe) may be NULL.
 *   - rt_hip_bake_probe_grid_depth: rt_hip_probe_grid_positions into the workspace, then rt_hip_bake_probe_depth at them;
 *     rt_hip_probe_grid_depth_workspace_bytes = the bake's own plus the positions (24 bytes a probe, after the bake's part).
 *
 * THE SHADE (rt_hip_probe_shade_vis): rt_hip_probe_shade's arguments, classes and steps 1 .. 7, with step 3 extended.  A corner whose
 * weight so far -- tri, times face with RT_HIP_GRID_FACING -- is == 0.0 is skipped as before, and its moments are not read either.
 * Otherwise, with C the corner's position (the grid's formula):
 *   p' = p + n*bias per component (the product rounded before the add); v = p' - C; q = (v.x*v.x + v.y*v.y) + v.z*v.z; r = sqrt(q).
 *   q > 0.0: (mean, mean2) = the lookup of probe i_c's map at v.  If r > mean: var = |mean*mean - mean2|; d = r - mean;
 *     ch = var / (var + d*d); ch = (ch*ch)*ch; vis_w = ch > floor ? ch : floor (a NaN ch, from 0/0, gives floor).  Otherwise
 *     vis_w = 1.0.  Then, if mean or mean2 is NaN, vis_w = a quiet NaN: an invalid probe poisons exactly the entries it would light.
 *   q == 0.0 (or NaN): vis_w = 1.0, and the moments are not read.
 *   w_c = w_c * vis_w.
 * Steps 4 to 7 follow with that w_c.  The function stays TOTAL: any bytes in d_moments give a defined result and no index leaves the
 * maps; for moments that are not NaN vis_w lies in [floor, 1], so that the weight sum of a VALID entry is never 0 where it was not
 * before.  With every mean >= every r it is rt_hip_probe_shade bit for bit (w_c * 1.0 = w_c).  The kernel reads the coefficients
 * through wave-uniform loads where a wave's valid entries share a cell, as k_probe_shade does, and the moments per lane: the same
 * operations in the same order in both arms, the same bits.
 *
 * THE PREVIEW.  rt_hip_probe_preview_vis is rt_hip_probe_preview with rt_hip_probe_shade_vis in the shade's place (the same
 * workspace: rt_hip_probe_preview_workspace_bytes); rt_hip_probe_preview_vis_image and _vis_scene_image are the host forms: they bake
 * the grid's coefficients (rt_hip_bake_probe_grid) and its moments (rt_hip_bake_probe_grid_depth) under probe_params, run the preview
 * and read back; h_moments (may be NULL) gets the moments.  Each is bit for bit the composition of the public calls.
 * Refusals, each before the first launch and with the outputs untouched, arguments before a device is looked for.  RT_HIP_EINVAL: a
 * NULL vis or a struct_size below the struct's; flags or reserved not 0; res outside 2 .. 32; sharp above 8; d_max not finite or not
 * > 0; bias not finite or negative; floor not finite or outside (0, 1]; n_probes * res * res > 2^28; a mode that is not
 * RT_HIP_PROBE_SPHERE; slice_rays == 0; a d_workspace that is not 16-byte aligned; a NULL required pointer; what rt_hip_bake_probes,
 * rt_hip_query_rays, rt_hip_probe_shade and rt_hip_probe_preview refuse.  n_probes == 0 or m == 0 with good arguments is RT_HIP_OK
 * and launches nothing. */
typedef struct
{
  uint32_t struct_size; /* set by rt_hip_probe_vis_defaults */
  uint32_t flags;       /* must be 0 */
  uint32_t res;         /* R: the map has R x R texels, 2 .. 32 */
  uint32_t sharp;       /* 0 .. 8: a ray weighs c^(2^sharp) in a texel */
  double d_max;         /* finite, > 0: distances are clamped to it, a miss counts as it */
  double bias;          /* finite, >= 0: the shaded point is moved along its normal by it */
  double floor;         /* finite, in (0, 1]: the least visibility weight */
  uint64_t reserved;    /* must be 0 */
} RtHipProbeVis;
void rt_hip_probe_vis_defaults(RtHipProbeVis *vis, const RtHipProbeGrid *grid);
size_t rt_hip_probe_depth_workspace_bytes(uint64_t n_probes, uint32_t res, uint32_t slice_rays);
int rt_hip_bake_probe_depth(const RtHipScene *scene, const double *d_positions, uint64_t n_probes, const RtHipProbeVis *vis,
                            const RtHipProbeParams *probe_params, uint32_t slice_rays, void *d_workspace, double *d_moments,
                            uint32_t *d_status, void *stream);
size_t rt_hip_probe_grid_depth_workspace_bytes(const RtHipProbeGrid *grid, uint32_t res, uint32_t slice_rays);
int rt_hip_bake_probe_grid_depth(const RtHipScene *scene, const RtHipProbeGrid *grid, const RtHipProbeVis *vis,
                                 const RtHipProbeParams *probe_params, uint32_t slice_rays, void *d_workspace, double *d_moments,
                                 uint32_t *d_status, void *stream);
int rt_hip_probe_shade_vis(const RtHipProbeGrid *grid, const RtHipProbeVis *vis, const double *d_coeff, const double *d_moments,
                           const double *d_points, const double *d_normals, const uint32_t *d_status, const float *d_albedo,
                           const float *d_add, uint64_t m, double *d_irradiance, float *d_color, void *stream);
int rt_hip_probe_preview_vis(const RtHipScene *scene, const RtHipCamera *camera, const RtHipProbeGrid *grid, const RtHipProbeVis *vis,
                             const double *d_coeff, const double *d_moments, int32_t width, int32_t height, int32_t aov_samples,
                             uint64_t seed, void *d_workspace, float *d_rgb, uint8_t *d_rgb8, void *stream);
int rt_hip_probe_preview_vis_image(const RtHipSphere *spheres, size_t n_spheres, const RtHipMesh *meshes, size_t n_meshes,
                                   const RtHipCamera *camera, const RtHipProbeGrid *grid, const RtHipProbeVis *vis,
                                   const RtHipProbeParams *probe_params, int32_t width, int32_t height, int32_t aov_samples, int device,
                                   float *h_rgb, uint8_t *h_rgb8, double *h_coeff, double *h_moments, uint64_t *h_stats);
int rt_hip_probe_preview_vis_scene_image(const RtHipScene *scene, const RtHipCamera *camera, const RtHipProbeGrid *grid,
                                         const RtHipProbeVis *vis, const RtHipProbeParams *probe_params, int32_t width, int32_t height,
                                         int32_t aov_samples, float *h_rgb, uint8_t *h_rgb8, double *h_coeff, double *h_moments,
                                         uint64_t *h_stats);

/* ---- probe updates: a grid that follows a moving scene, round by round, with hysteresis --------------------------------------------
 * A baked grid is a snapshot.  After rt_hip_scene_update_spheres or _vertices an UPDATE ROUND traces a few fresh rays for some of the
 * probes and blends them into the grid's STATE: its coefficients, its depth moments and an AGE a probe (a uint32: how many rounds have
 * updated the probe since it started over; 0 = it holds nothing yet).  The generator, the radiance and the ray query and the two folds
 * are called as they stand; what is new is a pure function of its arguments, stated here.  All arithmetic is fp64 + - * /, unfused,
 * in the order written.
 *
 * THE ROUND'S PROBES (RtHipProbeUpdate: stride >= 1, phase < stride).  With n the grid's probe count, the round updates the probes
 * i_j = phase + j*stride for j = 0 .. M-1, M = phase < n ? (n - 1 - phase) / stride + 1 : 0 (rt_hip_probe_update_count).  No list is
 * taken: no two writers can collide, and the function is total.
 * THE ROUND'S RAYS are those of rt_hip_bake_probes in RT_HIP_PROBE_SPHERE mode at the M positions of i_0 .. i_{M-1} (the grid's
 * formula), in that order, under probe_params with one change: seed_u = rt_mix64(seed + (uint64_t)round), a wrapping add and
 * rt_rng.h's rt_mix64.  So ray k = j*S + s, and the fresh sums are that call's d_sum bit for bit; with a vis the fresh W, M1, M2 are
 * the depth fold's sums ("probe visibility") of the very same rays.
 *
 * ALPHA of probe i.  a = age[i]; warm = 1.0 / ((double)a + 1.0); base = 1.0 - h; alpha = warm > base ? warm : base.  An age of 0 gives
 * alpha == 1.0: the probe STARTS OVER.  (h == 0.0 gives alpha == 1.0 at any age, and a probe of age >= 1 blends all the same.)
 * THE COEFFICIENT BLEND of an updated probe.  fresh[b][ch] = (sum[j][b][ch] * (1.0 / (double)S)) * K, S and K the resolve's own.
 *   age 0:         out = fresh; old is not read, so that uninitialised memory and a NaN state both recover; change_out = 1.0.
 *   otherwise:     c = 0.0, m = 0.0, and over ch = 0, 1, 2 of band 0: d = |fresh[0][ch] - old[0][ch]|; c = d > c ? d : c;
 *                  g = |fresh[0][ch]| > |old[0][ch]| ? |fresh[0][ch]| : |old[0][ch]|; m = g > m ? g : m (a NaN is passed over).
 *                  change_out = m > 0.0 ? c / m : 0.0.  The fast rule: if change > 0.0 && c > change * m then
 *                  alpha = alpha > (1.0 - fast) ? alpha : (1.0 - fast).  keep = 1.0 - alpha;
 *                  out[b][ch] = (old[b][ch] * keep) + (fresh[b][ch] * alpha).
 *   A NaN fresh sum (an invalid ray) makes the probe's coefficients NaN.  d_coeff_f, where given, gets (float)out; d_change, where
 *   given, change_out.
 * THE MOMENT BLEND of an updated probe, per texel, with the alpha by age alone (the fast rule does not apply); keep = 1.0 - alpha:
 *   W is NaN:    both moments become W.
 *   W > 0.0:     f = M1 / W, f2 = M2 / W; at age 0 out = (f, f2) and old is not read, else out = (old * keep) + (f * alpha), each
 *                moment.
 *   otherwise    (W == 0.0: the round says nothing about this texel) old stays bit for bit; at age 0 the texel gets
 *                (d_max, d_max*d_max), as the depth resolve gives.
 * THE AGE STEP, after both blends: age[i] = age[i] == 0xFFFFFFFF ? age[i] : age[i] + 1, for the round's probes only.
 * A probe that is not in the round keeps every bit of coeff, coeff_f, moments, age, change and status.  The status word of an updated
 * probe becomes the word rt_hip_bake_probes gives it in the round's bake.  That is 1: a round refuses a grid whose farthest position
 * origin[a] + (double)(count[a] - 1) * step[a] is not finite on some axis, so every position is finite, every generated direction is
 * a unit vector, and no ray of a round is invalid.  NaN sums reach the blends only through rt_hip_probe_blend_*, from a caller.
 *
 *   - rt_hip_probe_update_defaults: struct_size = sizeof(RtHipProbeUpdate), stride 1, phase 0, round 0, hysteresis 0.9, change 0,
 *     fast 0, flags and reserved 0.
 *   - rt_hip_probe_update_count: M; 0 for arguments any call would refuse.
 *   - rt_hip_probe_update_workspace_bytes: the d_workspace (16-byte aligned) of a round in slices of slice_rays rays: the bake's
 *     part for M probes, with a vis the depth bake's, the M positions and M status words; 0 for arguments any call would refuse.
 *   - rt_hip_probe_grid_update: the round on `stream` with no host wait; no output bit depends on slice_rays.  d_coeff (n x 9 x 3
 *     doubles) and d_age (n uint32) are required; d_moments (n x R*R x 2) is given iff vis is; d_coeff_f, d_change (a double a
 *     probe), d_status (a uint32 a probe) and d_stats (rt_hip_trace_rays' counters, added to) may be NULL.
 *   - rt_hip_probe_blend_coeff, _blend_moments, _age_step: the blends and the step alone, on sums the caller supplies by j (M x 9 x 3
 *     doubles; M x R*R x 3 doubles: W, M1, M2), asynchronous on `stream`, on the device that holds d_age.  M == 0 launches nothing.
 *   - rt_hip_probe_grid_update_host: the host form, synchronous, with a scene of its own on logical device `device`; h_coeff,
 *     h_moments (iff vis) and h_age are read and written, h_coeff_f, h_change and h_status (each may be NULL) written for the round's
 *     probes and otherwise as given; h_stats (may be NULL) is overwritten; it checks the device's status word (rt_hip_launch_status).
 *   - rt_hip_probe_update_preview_scene_image: for a host that holds a scene and a state across frames: the round
 *     (rt_hip_probe_grid_update) on the state in h_coeff, h_moments (iff vis) and h_age, read and written, then rt_hip_probe_preview
 *     (with a vis: rt_hip_probe_preview_vis) lit by the state the round leaves, seed = probe_params->seed, read back into h_rgb and
 *     h_rgb8 (either may be NULL, not both); synchronous, on the scene's device; h_stats (may be NULL) is overwritten with the
 *     round's counters; it checks the device's status word.  Bit for bit the composition of the two calls; it refuses what they do.
 * Refusals, each before any launch and with the outputs untouched, arguments before the device is looked for.  RT_HIP_EINVAL: a NULL
 * upd or a struct_size below the struct's; flags or reserved not 0; stride 0; phase >= stride; hysteresis or fast outside [0, 1) or
 * not finite; change negative or not finite; d_moments and vis not both given or both absent; a NULL d_age or d_coeff; a d_moments
 * that is not 16-byte aligned; a grid whose last position on an axis is not finite; samples < 1 for the blend; everything
 * rt_hip_bake_probe_grid and rt_hip_bake_probe_grid_depth refuse.  M == 0 is RT_HIP_OK and launches nothing. */
typedef struct
{
  uint32_t struct_size; /* set by rt_hip_probe_update_defaults */
  uint32_t flags;       /* must be 0 */
  uint32_t stride;      /* >= 1: a round updates the probes i with i % stride == phase */
  uint32_t phase;       /* < stride */
  uint32_t round;       /* u: picks the round's rays */
  uint32_t reserved;    /* 0 */
  double hysteresis;    /* h in [0, 1): share of the old state a warm probe keeps */
  double change;        /* finite, >= 0; 0 = off: relative change of the L0 band above which `fast` applies */
  double fast;          /* in [0, 1): the hysteresis of a probe whose change exceeds `change` */
} RtHipProbeUpdate;
void rt_hip_probe_update_defaults(RtHipProbeUpdate *upd);
uint64_t rt_hip_probe_update_count(const RtHipProbeGrid *grid, const RtHipProbeUpdate *upd);
size_t rt_hip_probe_update_workspace_bytes(const RtHipProbeGrid *grid, const RtHipProbeVis *vis, const RtHipProbeUpdate *upd,
                                           uint32_t slice_rays);
int rt_hip_probe_grid_update(const RtHipScene *scene, const RtHipProbeGrid *grid, const RtHipProbeVis *vis,
                             const RtHipProbeParams *probe_params, const RtHipProbeUpdate *upd, uint32_t slice_rays, void *d_workspace,
                             double *d_coeff, float *d_coeff_f, double *d_moments, uint32_t *d_age, double *d_change, uint32_t *d_status,
                             uint64_t *d_stats, void *stream);
int rt_hip_probe_blend_coeff(const double *d_sum, int32_t samples, const RtHipProbeGrid *grid, const RtHipProbeUpdate *upd,
                             const uint32_t *d_age, double *d_coeff, float *d_coeff_f, double *d_change, void *stream);
int rt_hip_probe_blend_moments(const double *d_sums, const RtHipProbeGrid *grid, const RtHipProbeVis *vis, const RtHipProbeUpdate *upd,
                               const uint32_t *d_age, double *d_moments, void *stream);
int rt_hip_probe_age_step(const RtHipProbeGrid *grid, const RtHipProbeUpdate *upd, uint32_t *d_age, void *stream);
int rt_hip_probe_grid_update_host(const RtHipSphere *spheres, size_t n_spheres, const RtHipMesh *meshes, size_t n_meshes,
                                  const RtHipProbeGrid *grid, const RtHipProbeVis *vis, const RtHipProbeParams *probe_params,
                                  const RtHipProbeUpdate *upd, int device, double *h_coeff, float *h_coeff_f, double *h_moments,
                                  uint32_t *h_age, double *h_change, uint32_t *h_status, uint64_t *h_stats);
int rt_hip_probe_update_preview_scene_image(const RtHipScene *scene, const RtHipCamera *camera, const RtHipProbeGrid *grid,
                                            const RtHipProbeVis *vis, const RtHipProbeParams *probe_params, const RtHipProbeUpdate *upd,
                                            int32_t width, int32_t height, int32_t aov_samples, float *h_rgb, uint8_t *h_rgb8, double *h_coeff,
                                            double *h_moments, uint32_t *h_age, uint64_t *h_stats);

/* ---- edge-avoiding a-trous denoiser guided by the first-hit buffers ---------------------------------------------------------
 * Inputs: row-major images of w x h pixels (1 <= w, h <= 2^20, w*h < 2^32) on one device -- colour c (3 floats per pixel: the
 * linear mean of rt_hip_render_tiles or rt_hip_accum_resolve after rt_hip_untile) and the RtHipAov buffers of the same frame
 * after rt_hip_untile_aov: albedo a (needed with DEMODULATE only), normal n, depth z, hits h, object o (with OBJECT_EDGES only).
 * All arithmetic is fp64 +, -, *, / in the order written; values read from float buffers are widened exactly; every stored
 * intermediate is rounded to float32 (RNE).  eps = 2^-10, h5 = [1/16, 1/4, 3/8, 1/4, 1/16] (index dx + 2).
 *   1. A pixel is INVALID if any channel of c is not finite: its output is its input colour, and no pixel uses it as a neighbour.
 *   2. e0 = float(c / (a + eps)) per channel with DEMODULATE, else e0 = c.
 *   3. For i = 0 .. L-1: step s = 2^i, sigma_i = sigma_color * 2^-i, S2 = sigma_i * sigma_i.  For each valid p, W = A = 0 (fp64);
 *      taps q = p + s*(dx, dy), dy = -2..2 (outer), dx = -2..2 (inner).  A tap outside the image or invalid is SKIPPED (not added:
 *      adding +0.0 would turn a -0.0 sum positive).  The centre tap has w = 9/64 and no edge terms.  Any other tap:
 *        - OBJECT_EDGES: skip q if o_q != o_p;
 *        - h_p == h_q == 0 (both background): wn = Zn = Zd = 1; exactly one of h_p, h_q is 0: skip q;
 *        - otherwise g = (n_p.x*n_q.x + n_p.y*n_q.y) + n_p.z*n_q.z, g = (g > 0) ? g : 0, wn = g squared k times;
 *          D = (sigma_depth * z_p) * (s * max(|dx|, |dy|)), Zn = D*D, dz = z_q - z_p, Zd = Zn + dz*dz; if Zd == 0: Zn = Zd = 1;
 *        - dc = ((de.x*de.x + de.y*de.y) + de.z*de.z) with de = e_q - e_p;
 *        - w = (((h5[dx]*h5[dy]) * wn) * (S2 * Zn)) / ((S2 + dc) * Zd);  W += w, then A += w * e_q per channel.
 *      e_{i+1}(p) = float(A / W) per channel (W >= 9/64).
 *   4. out = float(e_L * (a + eps)) with DEMODULATE, else e_L; invalid pixels pass c through.  out8 = the render epilogue's
 *      tonemap of the widened float.  L = 0 is allowed (without DEMODULATE it is the identity).
 * The contract is total: any buffer contents (NaN normals, a finite depth with 0 hits, ...) have a defined result.
 *   - rt_hip_denoise_defaults: L = 5, sigma_color = 0.5, k = 3, sigma_depth = 1.0, DEMODULATE.
 *   - rt_hip_denoise_workspace_bytes: the d_workspace rt_hip_denoise needs for w x h (0 for a size out of range).
 *   - rt_hip_denoise: asynchronous on `stream`, on the device that holds d_rgb.  d_aov: device image pointers (the ones the flags
 *     need); either output may be NULL, not both; d_out_rgb == d_rgb is allowed (in place).  Arguments are checked before the
 *     device is looked for: RT_HIP_EINVAL, then RT_HIP_ENODEV.
 *   - rt_hip_denoise_image: the same from host arrays, synchronous, with its own device buffers, on logical device `device` of
 *     rt_hip_render_image's device map (the HIP device itself without a map). */
typedef struct
{
  int32_t iterations;         /* L, 0 .. 10 */
  uint32_t flags;             /* RT_HIP_DENOISE_* */
  uint32_t normal_power_log2; /* k, 0 .. 10: the normal weight is max(0, n_p.n_q)^(2^k) */
  double sigma_color;        /* > 0, finite */
  double sigma_depth;         /* > 0, finite */
} RtHipDenoiseParams;
enum
{
  RT_HIP_DENOISE_DEMODULATE = 1u,   /* filter c / (albedo + eps), multiply the albedo back after */
  RT_HIP_DENOISE_OBJECT_EDGES = 2u, /* never mix pixels of different object ids */
};
void rt_hip_denoise_defaults(RtHipDenoiseParams *params);
size_t rt_hip_denoise_workspace_bytes(int32_t width, int32_t height);
int rt_hip_denoise(const float *d_rgb, const RtHipAov *d_aov, int32_t width, int32_t height, const RtHipDenoiseParams *params,
                   void *d_workspace, float *d_out_rgb, uint8_t *d_out_rgb8, void *stream);
int rt_hip_denoise_image(const float *h_rgb, const RtHipAov *h_aov, int32_t width, int32_t height, const RtHipDenoiseParams *params,
                         int device, float *h_out_rgb, uint8_t *h_out_rgb8);

/* ---- temporal reprojection: a frame's history carried across a camera move --------------------------------------------------
 * The step between two frames of a static scene: where was each pixel's first-hit point in the previous frame, is it the same
 * surface there, fetch the accumulated colour there, blend.  Inputs: row-major images of w x h pixels (2 <= w, h <= 2^20,
 * w*h < 2^32; the lower bound is that of the division by w - 1) on one device -- the frame's colour c (3 floats per pixel) and its
 * RtHipAov buffers after rt_hip_untile_aov (normal n, depth z, hits, object; albedo is ignored), the frame's camera; and the
 * HISTORY: the previous call's out_rgb and out_len, the previous frame's RtHipAov buffers and camera (primed names below; H, V,
 * llc, pos: a camera's horizontal, vertical, lower_left_corner, position).  d_hist_rgb, d_hist_len, d_hist_aov and hist_camera are
 * NULL together: the first frame.  Cameras are host pointers.
 * All arithmetic is fp64 +, -, *, /, sqrt, floor in the order written, unfused; values read from float buffers are widened exactly;
 * every stored value is rounded to float32 (RNE).  dot(a,b) = (a.x*b.x + a.y*b.y) + a.z*b.z;
 * cross(a,b) = (a.y*b.z - a.z*b.y, a.z*b.x - a.x*b.z, a.x*b.y - a.y*b.x).  Every comparison is false for NaN.  Per pixel p = (x, y):
 *   1. If any channel of c = rgb(p) is not finite: out = c, len = 0, motion = (qNaN, qNaN) with qNaN = 0x7FC00000.  Done.
 *   2. If there is no history (NULL), or hits(p) == 0, or !(z_p > 0 && z_p < +inf): out = c, len = 1, motion = qNaN.  Done.  (A
 *      background pixel needs no history: every sample of it is BACKGROUND.)
 *   3. The first-hit point, get_camera_ray (raytracer.c:375-384) operation for operation as the RT_HIP_RAYS_CAMERA_UV queries form it:
 *      u = (x + 0.5) / (w - 1.0), v = (y + 0.5) / (h - 1.0), E = llc + (H*u + V*v), d = vec3_normalize(pos - E) (m = sqrt(dot),
 *      then * (1.0 / m)), P = pos + d*z_p.
 *   4. Its place in the previous frame: D = P - pos', R = pos' - llc', N = cross(V', D), det = dot(H', N), us = dot(R, N) / det,
 *      M = cross(D, H'), vs = dot(R, M) / det, k = dot(R, cross(H', V')).  The point is in front iff (k > 0 && det > 0) ||
 *      (k < 0 && det < 0).  fx = us*(w - 1.0) - 0.5, fy = vs*(h - 1.0) - 0.5.  ok = in front && fx > -1 && fx < w && fy > -1 &&
 *      fy < h.  If !ok: out = c, len = 1, motion = qNaN.  Done.  Otherwise motion = (float(fx - x), float(fy - y)).
 *   5. x0 = floor(fx), a = fx - x0, y0 = floor(fy), b = fy - y0, zexp = sqrt(dot(D, D)), W = A = S = 0.  Taps j = 0, 1 (outer),
 *      i = 0, 1 (inner): q = (x0 + i, y0 + j) with weight wt = (i ? a : 1.0 - a) * (j ? b : 1.0 - b).  A tap is ACCEPTED iff q is
 *      inside the image, all three channels of hist_rgb(q) are finite, len'_q >= 1 && len'_q < +inf, hits'_q > 0,
 *      object'_q == object_p, dot(n_p, n'_q) >= normal_min and |z'_q - zexp| <= depth_tol * zexp.  An accepted tap: W += wt, then
 *      A += wt * hist_rgb(q) per channel, then S += wt * len'_q.  A rejected tap is SKIPPED, not added as zero.
 *   6. If !(W > 0): out = c, len = 1.  Otherwise hc = float(A / W) per channel, Nn = S / W + 1.0, if Nn > max_history: Nn =
 *      max_history, al = 1.0 / Nn, out = float(hc + (c - hc) * al) per channel, len = float(Nn).
 *   7. out8 = the render epilogue's tonemap of the widened out.
 * The contract is total: any buffer contents and any camera bytes (a degenerate or NaN camera, depths that are 0, negative or inf,
 * a zeroed history) have a defined result.  len = 0 marks a pixel the next frame must not use; a zero-filled history (buffers and
 * camera) behaves like no history.  Step 3 assumes a scene that is static between the two frames; after
 * rt_hip_scene_update_vertices the caller gives the previous points instead (rt_hip_reproject_points, below) and keeps the
 * history.  Moved spheres (rt_hip_scene_update_spheres) likewise: rt_hip_prev_points_moved.  Out of scope: topology changes, demodulated history, variance estimates.
 *   - rt_hip_reproject_defaults: flags 0, max_history = 32, depth_tol = 0.05, normal_min = 0.5 (DESIGN, "`pt_reproject`": the sweep).
 *   - rt_hip_reproject: asynchronous on `stream`, on the device that holds d_rgb.  d_out_rgb and d_out_len are required,
 *     d_out_rgb8 and d_out_motion (2 floats per pixel) may be NULL; d_out_rgb == d_rgb is allowed (in place).  No output may overlap
 *     a history buffer, another output, or a buffer of the frame in any other way (RT_HIP_EINVAL).  Arguments are checked before the device is looked for: RT_HIP_EINVAL, then RT_HIP_ENODEV.
 *     A call takes no pool, workspace or status word.
 *   - rt_hip_reproject_image: the same from host arrays, synchronous, with its own device buffers, on logical device `device` of
 *     rt_hip_render_image's device map (the HIP device itself without a map). */
typedef struct
{
  uint32_t flags;     /* must be 0 */
  double max_history; /* >= 1, finite: cap of the history length N */
  double depth_tol;   /* >= 0, finite: relative depth tolerance */
  double normal_min;  /* finite: least n_p . n'_q of an accepted tap */
} RtHipReprojectParams;
void rt_hip_reproject_defaults(RtHipReprojectParams *params);
int rt_hip_reproject(const float *d_rgb, const RtHipAov *d_aov, const RtHipCamera *camera, const float *d_hist_rgb,
                     const float *d_hist_len, const RtHipAov *d_hist_aov, const RtHipCamera *hist_camera, int32_t width, int32_t height,
                     const RtHipReprojectParams *params, float *d_out_rgb, uint8_t *d_out_rgb8, float *d_out_len, float *d_out_motion,
                     void *stream);
int rt_hip_reproject_image(const float *h_rgb, const RtHipAov *h_aov, const RtHipCamera *camera, const float *h_hist_rgb,
                           const float *h_hist_len, const RtHipAov *h_hist_aov, const RtHipCamera *hist_camera, int32_t width,
                           int32_t height, const RtHipReprojectParams *params, int device, float *h_out_rgb, uint8_t *h_out_rgb8,
                           float *h_out_len, float *h_out_motion);

/* ---- reprojection across vertex updates: previous points per pixel -----------------------------------------------------------
 * After rt_hip_scene_update_vertices the surface under a pixel was somewhere else one frame ago, and step 3 above, which rebuilds
 * the first-hit point from today's geometry, looks the history up where the surface was not.  Two calls close the gap: a
 * RT_HIP_RAYS_CAMERA_UV query through the pixel centres gives each pixel's triangle and barycentrics; rt_hip_prev_points blends
 * the triangle's PREVIOUS corners with them; rt_hip_reproject_points starts from that point.
 *
 * rt_hip_prev_points: d_hits as rt_hip_query_rays fills it (status, prim, bary and point are required, the other fields are not
 * read), n entries (0 <= n < 2^32); d_positions: 9 doubles per triangle (v0, v1, v2) in scene triangle order -- the layout of
 * rt_hip_scene_update_vertices, the numbering of the query's prim --, the positions the scene had at the previous frame
 * (n_triangles may be 0, d_positions then NULL); d_points: 3 doubles per entry.  fp64 +, -, *, unfused, in the order written.  Entry i:
 *   - status != 1: three quiet NaNs, bits 0x7FF8000000000000;
 *   - status == 1 and prim == 0xFFFFFFFF (a sphere; one that moved: rt_hip_prev_points_moved): the three words of point, copied as bits;
 *   - status == 1 and prim < n_triangles: u = bary[0], v = bary[1], w0 = (1.0 - u) - v, out_k = (a_k*w0 + b_k*u) + c_k*v for
 *     k = x, y, z with a, b, c the triangle's corners -- the blend intersect_triangle applies to the texture coordinates
 *     (raytracer.c:158-164), applied to positions;
 *   - any other prim: three quiet NaNs.
 * The contract is total: any bits in any input have a defined result (overflow to inf is a result; a NaN that the blend's own
 * arithmetic makes is a NaN, its sign and payload the machine's).  d_points == d_hits->point is
 * allowed (a lane reads its own point before it writes); any other overlap of d_points with an input is RT_HIP_EINVAL.
 * Asynchronous on `stream`, on the device that holds d_points.  Arguments are checked before the device is looked for:
 * RT_HIP_EINVAL, then RT_HIP_ENODEV.  n == 0 is RT_HIP_OK and launches nothing.  A call takes no pool, workspace or status word.
 * rt_hip_prev_points_host: the same from host arrays, synchronous, with buffers of its own, on logical device `device` of
 * rt_hip_render_image's device map.
 *
 * rt_hip_reproject_points: rt_hip_reproject's arguments and d_prev_points.  NULL: the call is rt_hip_reproject itself, the same
 * kernel and the same bits.  Otherwise 3 doubles per pixel, row-major, and the contract is rt_hip_reproject's with step 3 replaced:
 *   3'. P = prev_points(p).  If a component of P is not finite: out = c, len = 1, motion = qNaN.  Done.  (No surface to look up: a
 *       disocclusion, a miss, an invalid ray.)  The frame's camera is not read in this form.
 * Steps 1, 2 and 4-7 are unchanged with D = P - pos': zexp is the previous point's distance from the previous camera, and motion
 * is the true screen-space motion, the surface's own included.  Parameters, ranges and overlap rules are rt_hip_reproject's;
 * d_prev_points must not overlap any output (RT_HIP_EINVAL).  rt_hip_reproject_points_image: the same from host arrays.
 *
 * rt_hip_prev_points_moved: rt_hip_prev_points after rt_hip_scene_update_spheres.  d_hits->object is required as well; d_spheres_prev
 * and d_spheres_cur: 4 doubles per sphere (cx, cy, cz, radius) in object order, the spheres at the previous frame and now.  The
 * contract above holds word for word for triangles, for status != 1 and for out-of-range prims.  A sphere hit, status == 1 and prim
 * == 0xFFFFFFFF:
 *   - object < n_spheres: with (c', r') the previous sphere and (c, r) the current one, s = r' / r, then
 *     out_k = c'_k + (point_k - c_k) * s for k = x, y, z -- fp64, unfused, in that order: the surface point rides the sphere's
 *     translation and uniform scale (a sphere has no orientation in this scene model);
 *   - object >= n_spheres: three quiet NaNs;
 *   - d_spheres_prev == NULL and n_spheres == 0: the three words of point, copied as bits -- the call is rt_hip_prev_points itself.
 * With n_spheres != 0 both arrays are required (RT_HIP_EINVAL); they and object must not overlap d_points.  Totality, the overlap
 * rule, the error order and n == 0 are rt_hip_prev_points'.  rt_hip_reproject_points is fed unchanged. */
int rt_hip_prev_points(const RtHipHits *d_hits, uint64_t n, const double *d_positions, size_t n_triangles, double *d_points, void *stream);
int rt_hip_prev_points_host(const RtHipHits *h_hits, uint64_t n, const double *h_positions, size_t n_triangles, int device,
                            double *h_points);
int rt_hip_prev_points_moved(const RtHipHits *d_hits, uint64_t n, const double *d_positions, size_t n_triangles,
                             const double *d_spheres_prev, const double *d_spheres_cur, size_t n_spheres, double *d_points, void *stream);
int rt_hip_prev_points_moved_host(const RtHipHits *h_hits, uint64_t n, const double *h_positions, size_t n_triangles,
                                  const double *h_spheres_prev, const double *h_spheres_cur, size_t n_spheres, int device, double *h_points);
int rt_hip_reproject_points(const float *d_rgb, const RtHipAov *d_aov, const RtHipCamera *camera, const float *d_hist_rgb,
                            const float *d_hist_len, const RtHipAov *d_hist_aov, const RtHipCamera *hist_camera, int32_t width,
                            int32_t height, const RtHipReprojectParams *params, const double *d_prev_points, float *d_out_rgb,
                            uint8_t *d_out_rgb8, float *d_out_len, float *d_out_motion, void *stream);
int rt_hip_reproject_points_image(const float *h_rgb, const RtHipAov *h_aov, const RtHipCamera *camera, const float *h_hist_rgb,
                                  const float *h_hist_len, const RtHipAov *h_hist_aov, const RtHipCamera *hist_camera, int32_t width,
                                  int32_t height, const RtHipReprojectParams *params, const double *h_prev_points, int device,
                                  float *h_out_rgb, uint8_t *h_out_rgb8, float *h_out_len, float *h_out_motion);

/* ---- guided upsampling: a full-size frame from a low-resolution render -------------------------------------------------------
 * Joint bilateral upsampling (Kopf et al. 2007): the colour is rendered (and denoised) at a fraction of the size and brought to
 * full size under the full-resolution first-hit buffers, which are cheap and exact; with DEMODULATE the texture detail and the
 * silhouettes come from those guides, not from the colour.  Inputs: row-major images on one device -- the LOW frame of wl x hl
 * pixels (primed names: colour c', 3 floats per pixel, and its RtHipAov buffers after rt_hip_untile_aov) and the guides, the
 * RtHipAov buffers of the HIGH frame of w x h pixels; 2 <= w, h, wl, hl <= 2^20 and w*h, wl*hl < 2^32 (the lower bound is that of
 * the division by w - 1).  Any ratio is allowed, not only integer ones and not only wl < w.  Both frames are of the same scene
 * under the same camera struct (init_camera depends on the aspect ratio only, and get_camera_ray's (x + r) / (w - 1) ties the two
 * pixel grids together).  Fields read, at both sizes: normal n, depth z and hits always; albedo with DEMODULATE; object with
 * OBJECT_EDGES.
 * All arithmetic is fp64 +, -, *, /, floor in the order written, unfused; values read from float buffers are widened exactly;
 * every stored value is rounded to float32 (RNE).  eps = 2^-10.  dot(a,b) = (a.x*b.x + a.y*b.y) + a.z*b.z.  Every comparison is
 * false for NaN.  Per HIGH pixel p = (x, y):
 *   1. Its place in the low frame: fx = ((x + 0.5) * (wl - 1.0)) / (w - 1.0) - 0.5, fy likewise with h and hl (with equal sizes
 *      this is exactly x).  x0 = floor(fx), a = fx - x0, y0 = floor(fy), b = fy - y0.
 *   2. Taps j = 0, 1 (outer), i = 0, 1 (inner): q = (x0 + i, y0 + j) with weight wt = (i ? a : 1.0 - a) * (j ? b : 1.0 - b).
 *      e_q = float(c'_q / (albedo'_q + eps)) per channel with DEMODULATE, otherwise e_q = c'_q.  A tap is USABLE iff q is inside
 *      the low image, wt > 0, and all three channels of e_q are finite.
 *   3. The guide weight g of a usable tap.  hits_p == 0 and hits'_q == 0: g = 1.  Exactly one of them 0: g = 0.  Otherwise: with
 *      OBJECT_EDGES and object'_q != object_p, g = 0; otherwise d = dot(n_p, n'_q), d = (d > 0) ? d : 0, wn = d squared k times,
 *      D = sigma_depth * z_p, Zn = D*D, dz = z'_q - z_p, Zd = Zn + dz*dz, if Zd == 0: Zn = Zd = 1, g = (wn * Zn) / Zd.
 *      om = wt * g.  The tap is ACCEPTED iff om > 0 && om < +inf (a NaN guide therefore rejects): W += om, then A += om * e_q per
 *      channel, both from 0.  A tap that is not accepted is SKIPPED, not added as zero.
 *   4. The blend.  W > 0: e = float(A / W) per channel and conf = float(W / U), where U is the sum of wt over the usable taps,
 *      added in tap order from 0.  Otherwise the FALLBACK, plain bilinear over the usable taps: e = float(A2 / U) with A2 += wt *
 *      e_q (tap order, from 0), and conf = 0.  No usable tap: e = 0 per channel and conf = -1.
 *   5. out = float(e * (albedo_p + eps)) per channel with DEMODULATE, otherwise e.  out8 = the render epilogue's tonemap of the
 *      widened out.
 * The contract is total: any buffer contents have a defined result.  conf marks where the low frame held no matching surface
 * (features and silhouettes finer than a low pixel): 1 where every usable tap matched fully, 0 where none did and the result is
 * plain bilinear, -1 where the low frame had nothing to give.  A caller can resample exactly those pixels (rt_hip_trace_rays with
 * RT_HIP_RAYS_CAMERA_UV); that fill is not part of this call.
 *   - rt_hip_upsample_defaults: DEMODULATE, k = 3 (the denoiser's), sigma_depth = 0.05 (DESIGN, "`pt_upsample`").
 *   - rt_hip_upsample: asynchronous on `stream`, on the device that holds d_low_rgb.  d_out_rgb is required, d_out_rgb8 and
 *     d_out_conf (1 float per pixel) may be NULL.  No output may overlap an input or another output (RT_HIP_EINVAL).  Arguments are
 *     checked before the device is looked for: RT_HIP_EINVAL, then RT_HIP_ENODEV.  A call takes no pool, workspace or status word.
 *   - rt_hip_upsample_image: the same from host arrays, synchronous, with its own device buffers, on logical device `device` of
 *     rt_hip_render_image's device map (the HIP device itself without a map). */
typedef struct
{
  uint32_t flags;             /* RT_HIP_UPSAMPLE_* */
  uint32_t normal_power_log2; /* k, 0 .. 10: the normal weight is max(0, n_p.n'_q)^(2^k) */
  double sigma_depth;         /* > 0, finite: the depth weight's width, relative to z_p */
} RtHipUpsampleParams;
enum
{
  RT_HIP_UPSAMPLE_DEMODULATE = 1u,   /* interpolate c' / (albedo' + eps), multiply the full-size albedo back after */
  RT_HIP_UPSAMPLE_OBJECT_EDGES = 2u, /* never take a tap of another object id */
};
void rt_hip_upsample_defaults(RtHipUpsampleParams *params);
int rt_hip_upsample(const float *d_low_rgb, const RtHipAov *d_low_aov, int32_t low_width, int32_t low_height, const RtHipAov *d_aov,
                    int32_t width, int32_t height, const RtHipUpsampleParams *params, float *d_out_rgb, uint8_t *d_out_rgb8,
                    float *d_out_conf, void *stream);
int rt_hip_upsample_image(const float *h_low_rgb, const RtHipAov *h_low_aov, int32_t low_width, int32_t low_height,
                          const RtHipAov *h_aov, int32_t width, int32_t height, const RtHipUpsampleParams *params, int device,
                          float *h_out_rgb, uint8_t *h_out_rgb8, float *h_out_conf);

/* ---- pixel refinement: resample only the pixels a mask selects -----------------------------------------------------------------
 * The upsampling's conf, the reprojection's len and any other per-pixel map say where a frame is not trustworthy yet.  Three calls
 * act on such a map on the device: SELECT the pixels, TRACE them with the samples render() itself would give them, BLEND the result
 * into the frame.  Each has a total contract of its own and they share nothing but the index list.
 *
 * rt_hip_select_pixels: the ordered compaction of a map.  d_values: one float per pixel, row-major, w x h with 1 <= w, h <= 2^20 and
 * n = w*h < 2^32.  Pixel p is SELECTED iff (lo <= v_p && v_p <= hi), negated under RT_HIP_SELECT_INVERT; lo and hi are doubles and
 * may be +-inf, v_p is widened exactly, a comparison is false for NaN (a NaN value is selected under INVERT only), -0.0 equals 0.0,
 * lo > hi selects nothing (everything under INVERT).  A NaN bound: RT_HIP_EINVAL.
 *   d_indices  uint32[capacity]: the selected p = y*w + x in strictly ascending order, the first min(count, capacity) of them;
 *              entries beyond that are left untouched.  capacity == 0 with d_indices == NULL only counts.
 *   d_count    one uint32: the full count, also when it exceeds capacity.
 * d_workspace: rt_hip_select_workspace_bytes(w, h) bytes (0 for a size out of range).  Asynchronous on `stream`, on the device that
 * holds d_values; no pool, no status word.  Arguments are checked before the device is looked for: RT_HIP_EINVAL, then RT_HIP_ENODEV.
 * Separate launches on the stream: per-workgroup counts (wave ballot + popcount, 256 pixels per workgroup), their exclusive scan
 * (1,024 counts per workgroup and level, the levels looped on the host: three levels hold 2^30 counts), a scatter by ballot prefix.
 * No workgroup waits on another inside a launch, so the result does not depend on scheduling.
 *
 * rt_hip_trace_pixels: render()'s own samples for a list of pixels.  The frame is params->width x height (2 <= w, h <= 2^20,
 * w*h < 2^32: rt_hip_render_tiles' limits) under `camera` (a host pointer); d_pixels is uint32[n], 0 <= n < 2^32, n a host value,
 * any order, duplicates allowed.  Entry i names pixel p = d_pixels[i], x = p % w, y = p / w, and is INVALID (status 2, zeros, as an
 * invalid ray) iff p >= w*h.  Sample k (0 <= k < S = params->samples) of a valid entry is THE RENDER'S SAMPLE s = sample_first + k OF
 * PIXEL p: the stream (seed, p, s) of rt_rng.h, its first two draws r0, r1 the jitter, the ray get_camera_ray(camera, (x + r0) /
 * (w - 1), (y + r1) / (h - 1)) formed operation for operation as the render kernels form it, the value trace_path(&ray, scene, n, 0)
 * at MAX_DEPTH = params->max_depth.  sample_first >= 0 and sample_first + S <= 2^31.
 * The mean has rt_hip_trace_rays' shape with slice = k mod 4: S_j (j = 0 .. 3) is the ascending vec3_add, from +0.0, of the samples
 * with k = j (mod 4); total = (S_0 + S_1) + (S_2 + S_3); radiance = total * (1.0 / (double)S).
 * Outputs: RtHipRadiance (status, radiance, samples entry-major [i*S + k], paths, casts: each may be NULL, not all; ray must be
 * NULL).  d_stats (RT_HIP_NSTATS accumulators, may be NULL) += the render's four counters: rays = the sum of paths, casts, tests =
 * casts x primitives, samples = valid entries x S.
 * Exactness, as for radiance queries: every decision is the reference's, so `paths` and `casts` per entry equal the compiled
 * reference's trace_sample(scene, x, y, sample_first + k, seed) exactly; each sample VALUE is the render kernels' iteration, within
 * 2^-40 |ref| of it (with M_REFRACTION 2^-40 (|ref| + the entry's largest |ref|)).  Bit-exact are:
 *   (a) radiance is the stated reduction of samples;
 *   (b) an entry's outputs are a function of (scene, camera, w, h, seed, p, sample_first, S) alone: not of its position in the list,
 *       of the other entries, or of how the list is split over calls; a duplicate index gets duplicate bits;
 *   (c) a sample is a function of (scene, camera, w, h, seed, p, s) alone: S = 8, sample_first = 0 gives in samples 4 .. 7 the bits
 *       S = 4, sample_first = 4 gives.  Refining a frame of N spp with sample_first = N takes exactly the samples a progressive
 *       accumulation would take next, and re-draws none the frame already has.
 * Everything else is rt_hip_trace_rays': the two-child forms through the per-device pending-ray pool, the device's status word
 * (rt_hip_launch_status), NaN radiance and samples for the valid entries of a workgroup without its slot, max_depth 0 .. 1000000 and
 * <= 32 with M_REFRACTION (RT_HIP_ELIMIT), integrator RT_HIP_TRACE_PATH only, the error order, n == 0 launching nothing.
 *   - rt_hip_pixel_defaults: zeros, samples 1, max_depth 5, RT_HIP_TRACE_PATH (width and height are the caller's to set).
 *   - rt_hip_trace_pixels_host: the same from host arrays, synchronous, with a scene and buffers of its own, on logical device
 *     `device` of rt_hip_render_image's device map; h_stats (may be NULL) += the counters.
 *   - rt_hip_pixel_kernel_name / _count / _launches: the five forms (pt_trace_pixels[_big|_tri|_tri_big|_mem], picked as the
 *     radiance-query forms are; not members of the family of rt_hip_kernel_count) and the launches this process has made of each.
 *
 * rt_hip_blend_pixels: the new samples into the frame.  All arithmetic is fp64 + - * / in the order written, floats are widened
 * exactly, stores are rounded to float32 (RNE).  d_pixels[n] as the select gives them -- DISTINCT (with duplicates which entry wins
 * a pixel is unspecified; nothing faults); d_status and d_radiance of a trace call over that list; new_weight (finite, > 0,
 * typically S); prior_scale (>= 0, not NaN); d_prior (one float per pixel; NULL: 1.0 everywhere); the frame d_rgb (3 floats per
 * pixel of w x h, 1 <= w, h <= 2^20, w*h < 2^32), updated in place.  Per entry with p < w*h and status == 1 and all three channels
 * of r = radiance finite:
 *   1. wa = prior_scale * prior_p.
 *   2. If !(wa > 0), or wa is not finite, or a channel of c = rgb(p) is not finite: out = float(r), W = new_weight.
 *   3. Otherwise W = wa + new_weight, out = float((c * wa + r * new_weight) / W) per channel.
 * Any other entry leaves its pixel untouched.  Written at the touched pixels only: d_rgb; d_rgb8 (may be NULL), the render
 * epilogue's tonemap of the widened out; d_weight (may be NULL; may be d_prior itself), float(W).  The contract is total.  One
 * launch on `stream`, on the device that holds d_rgb; no pool, no workspace; n == 0 launches nothing.  RT_HIP_EINVAL, then
 * RT_HIP_ENODEV. */
enum
{
  RT_HIP_SELECT_INVERT = 1u
};
typedef struct
{
  int32_t width, height;  /* the frame the indices are of */
  int32_t samples;        /* S >= 1 */
  int32_t sample_first;   /* s0 >= 0, s0 + S <= 2^31 */
  int32_t max_depth;      /* the reference's MAX_DEPTH */
  uint32_t integrator;    /* must be RT_HIP_TRACE_PATH */
  uint64_t seed;
} RtHipPixelParams;
size_t rt_hip_select_workspace_bytes(int32_t width, int32_t height);
int rt_hip_select_pixels(const float *d_values, int32_t width, int32_t height, double lo, double hi, uint32_t flags, void *d_workspace,
                         uint32_t *d_indices, uint32_t capacity, uint32_t *d_count, void *stream);
void rt_hip_pixel_defaults(RtHipPixelParams *params);
int rt_hip_trace_pixels(const RtHipScene *scene, const RtHipCamera *camera, const uint32_t *d_pixels, uint64_t n,
                        const RtHipPixelParams *params, const RtHipRadiance *d_out, uint64_t *d_stats, void *stream);
int rt_hip_trace_pixels_host(const RtHipSphere *spheres, size_t n_spheres, const RtHipMesh *meshes, size_t n_meshes,
                             const RtHipCamera *camera, const uint32_t *h_pixels, uint64_t n, const RtHipPixelParams *params, int device,
                             const RtHipRadiance *h_out, uint64_t *h_stats);
const char *rt_hip_pixel_kernel_name(const RtHipScene *scene);
int rt_hip_pixel_kernel_count(void);
const char *rt_hip_pixel_kernel_launches(int index, uint64_t *launches);
int rt_hip_blend_pixels(const uint32_t *d_pixels, const uint32_t *d_status, const double *d_radiance, uint64_t n, int32_t width,
                        int32_t height, double new_weight, double prior_scale, const float *d_prior, float *d_rgb, uint8_t *d_rgb8,
                        float *d_weight, void *stream);

/* Scatter a compact tile buffer into row-major images (either output may be
 * NULL together with its input). */
int rt_hip_untile(const float *d_tiles_rgb, const uint8_t *d_tiles_rgb8, int32_t width, int32_t height,
                  uint32_t tile_first, uint32_t tile_stride, uint32_t tile_count, float *d_image_rgb,
                  uint8_t *d_image_rgb8, void *stream);

/* ---- self-test hook --------------------------------------------------------------- */

/* Evaluates one of the kernel's exact-arithmetic building blocks on host arrays (n values
 * each) so that tests can compare it bit for bit with IEEE results computed on the host:
 * op 0 sqrt without range scaling (valid for 0 or >= 2^-767), 1 quotient by a small integer
 * through its reciprocal, 2 library sqrt, 3 IEEE division, 4 the fused r*2^-30 - 1 mapping,
 * 5 reciprocal without range scaling (valid for 2^-500 <= a <= 2^500), 6 the tabulated atan2 (a, b), 7 frac1 = fmod(a, 1.0),
 * 8 win_add of every a[i] into the windowed accumulator out[0..6) as h_out holds it on entry (n >= 8; out[6] counts refused
 * terms), 9 win_normalize + win_value of groups of six words (bit patterns in h_a[8g..8g+6); n a multiple of 8) -> h_out[8g..8g+6)
 * the normalised words, h_out[8g+6] the value. */
int rt_hip_selftest_math(int op, const double *h_a, const double *h_b, double *h_out, size_t n, int device);

/* Runs the render kernels' own exact primitive tests (intersect_sphere raytracer.c:77-118,
 * intersect_triangle :120-174 as the device states them) and their conservative phase-1
 * filter on host arrays, one GPU lane per case, so that known-answer vectors reach the device
 * code itself.  kind 0: h_prims = n x 4 (cx cy cz radius); kind 1: h_prims = n x 9 (v0 v1 v2
 * positions); h_rays = n x 6 (origin, direction).  Case i = ray i against primitive i:
 * h_hit[i] 0/1 and h_tuv[3i..] = t (DBL_MAX on a miss) and, for triangles, the barycentric
 * u, v (a texture coordinate is st0 (1-u-v) + st1 u + st2 v, raytracer.c:154-167).
 * h_keep[3i + f], f = 0..2: 64-bit masks of the filter's three forms (f = 0: spheres, sign tests
 * from LDS; triangles, the per-lane fp32 Moeller-Trumbore pre-test that follows the bounding-sphere
 * filter in small scenes; f = 1: compares from LDS; f = 2: compares by scalar loads) for ray i
 * against the 64 primitives of its block [64 (i/64), +64): bit j set = primitive 64 (i/64) + j
 * is kept.  The filter is built for ray origins within near_R (rays beyond keep everything),
 * as rt_hip_render_tiles builds it for a camera.  |centre|, |radius| <= 1e17.
 * kind 2 (spheres as kind 0, n a multiple of 64; a build with -DPT_MFMA16=0 refuses it): the keep words of phase 1 on the fp16
 * matrix pipe.  In each block of 64 cases the first 32 spheres are the matrix rows and the other 32 follow in the packed loop, as
 * in a scene of more than 32 small spheres.  h_keep[3i + 0] = the packed sign-test form alone, h_keep[3i + 1] = the matrix pipe
 * merged with it as the render kernels merge them, h_keep[3i + 2] = the device's exact test of ray i against the block's 64
 * spheres (bit j = a hit).  h_hit[i] = 1 when the block's 32 rows fit the matrix form (0: it ran the packed loop instead).
 * h_tuv[3i], h_tuv[3i + 1] = the matrix pipe's raw tca16 and ll16 of ray 64 (i/64) + i % 32 and sphere 64 (i/64) + 16 ((i % 64) / 32). */
int rt_hip_selftest_intersect(int kind, const double *h_rays, const double *h_prims, size_t n, double near_R,
                              uint8_t *h_hit, double *h_tuv, uint64_t *h_keep, int device);

/* Fault injection: from now on the named optional device allocations of the shim behave as if hipMalloc had failed, so that
 * the fallback rows of the pick table (no parked-walk workspace: the lane-waiting kernels; no pending-ray pool of 4 x 512 stacks
 * per slot: the static kernel of the family) are reachable on a device with 288 GB.  0 switches it off.  A scene that has
 * already met its workspace keeps it. */
enum
{
  RT_HIP_FAIL_ALLOC_PARK_WS = 1,
  RT_HIP_FAIL_ALLOC_WIDE_PEND = 2,
  RT_HIP_FAIL_ALLOC_TAIL_WS = 4 /* the mixed grid's workspace (rt_hip_mixed_grid_launches): the launch stays uniform */
};
void rt_hip_selftest_fail_alloc(uint32_t mask);

/* How many launches of this process took the MIXED GRID: rt_hip_render_tiles (one chunk, no workspace) of many rounds of workgroups
 * on pt_render_tiles runs the frame's last tiles as sample chunks behind the whole ones, in the same launch, so that the device
 * stays full to the frame's end; the frame, the bytes and the counters are the uniform launch's bit for bit.  The chunked tiles'
 * sums live in a small per-device workspace of the shim's (2 MB on an MI355X; rt_hip_release_cache() frees it).
 * RT_HIP_GRID_UNIFORM=1 in the environment keeps every launch uniform; RT_HIP_GRID_SPLIT=<whole tiles>,<chunks> sets the split
 * of every launch whose form takes one (tests, sweeps). */
uint64_t rt_hip_mixed_grid_launches(void);

/* How many slots per XCD the two per-device pools get on `device` (the parked-walk workspace, the pending-ray pool): CUs per
 * XCD x the most workgroups of any slot-taking kernel a CU can hold, + 25 %, rounded up to a multiple of 32. */
int rt_hip_selftest_pool_slots(int device, uint32_t *park_slots_per_xcd, uint32_t *pend_slots_per_xcd);

/* Launches n_workgroups one-wave workgroups; h_counts[x] = how many of them read HW_REG_XCC_ID == x
 * (bits 3:0).  The parked-walk kernels partition their workspace by that id (every owner a slot ever
 * has must sit behind the same L2): on an MI355X the counts must be spread over ids 0..7. */
int rt_hip_selftest_xcc(uint32_t n_workgroups, uint32_t h_counts[16], int device);

/* ---- convenience for C hosts: whole image, host buffers, synchronous ----------- */

/* Cooperative cancellation of rt_hip_render_image(): while a flag is registered, long frames
 * are rendered in slabs and *flag is polled between them (set it from a signal handler).  On
 * cancellation the finished tiles are still gathered and copied out, the rest of the image is
 * zero, and the call returns RT_HIP_ECANCELLED.  NULL unregisters. */
void rt_hip_set_cancel_flag(const volatile int *flag);

/* Renders width x height on n_devices GPUs of this process (tiles interleaved
 * over devices: logical device g renders tiles g, g + n_devices, ...; the compact tile buffers
 * are gathered onto logical device 0, scattered to the row-major image there and copied to the
 * host).  Calls are serialised (one frame at a time).  A segment travels by grouped ncclSend /
 * ncclRecv over cached communicators when its device differs from the root's, and as a
 * device-to-device copy when it does not (see rt_hip_set_device_map).
 * n_devices > 1 is EXPERIMENTAL in one respect only: its indexing, slabs, cancellation, caching
 * and counters run in the GPU tests at 2, 3 and 8 LOGICAL devices mapped onto one GPU, and its
 * RCCL calls run there with one rank (RT_HIP_FORCE_COMM=1) -- but as of this writing no machine
 * with two physical GPUs has run it; `bench.py --gpus N` exercises it in a child process whenever
 * N > 1 GPUs are present and compares its frame with the one-device frame.
 * h_image_rgb (w*h*3 floats) and
 * h_image_rgb8 (w*h*3 bytes) may each be NULL.  h_stats: RT_HIP_NSTATS values,
 * overwritten.  kernel_seconds: device time of the render kernels (max over
 * devices), may be NULL.  params->tile_* are ignored. */
int rt_hip_render_image(const RtHipSphere *spheres, size_t n_spheres, const RtHipMesh *meshes,
                        size_t n_meshes, const RtHipCamera *camera, const RtHipParams *params,
                        int n_devices, float *h_image_rgb, uint8_t *h_image_rgb8, uint64_t *h_stats,
                        double *kernel_seconds);

/* rt_hip_render_image() keeps what it built -- per-device scenes, streams, tile buffers, the RCCL
 * communicators -- and reuses it while the device count, the image size and the scene's bytes
 * stay the same (a caller rendering frame after frame re-creates nothing).  This releases it, and
 * with it the per-device pool of pending-ray stacks that scenes with two-child materials
 * (M_REFRACTION under trace_path, M_REFLECTION | M_REFRACTION under cast_ray) render with;
 * rt_hip_cache_builds() counts how often a context had to be (re)built (for tests). */
void rt_hip_release_cache(void);
uint64_t rt_hip_cache_builds(void);

/* What the shim holds on `device` besides scenes and frames, bytes (0: not allocated): the parked-walk workspace (scenes with a
 * mesh hierarchy; freed with the last such scene) and the pending-ray pool (two-child materials; grows to the deepest and widest
 * launch, is rebuilt to fit after 16 launches in a row needed at most a quarter of a pool above 1 GB, freed by
 * rt_hip_release_cache()).  INTEGRATION.md has the sizes.  Two small per-device allocations are NOT reported here: the 256 B status
 * word and the mixed grid's chunk records (rt_hip_mixed_grid_launches: one round of workgroups x 1.5 KB, 2 MB on an MI355X). */
int rt_hip_pool_bytes(int device, size_t *park_ws_bytes, size_t *pend_pool_bytes);

/* Where the host time of the last rt_hip_render_image() went, seconds: [0] context (scene compare; on a rebuild: upload,
 * buffers, workspaces, communicators), [1] launches + kernels + gather + scatter until every stream is idle, [2] the frame,
 * bytes and counters over PCIe. */
void rt_hip_last_image_phases(double seconds[3]);

/* Logical -> physical device map of rt_hip_render_image(): with a map of n entries, n_devices may be up to n and logical
 * device g runs on HIP device map[g]; entries may repeat.  Logical devices that share a physical one keep separate scenes,
 * streams and tile buffers (their kernels run concurrently on it); the partition, the slabs, the gather's slot arithmetic,
 * the per-segment scatter and the counter sums are the code that runs with n distinct GPUs, so a one-GPU machine executes
 * the whole n_devices > 1 path (map = {0, 0, 0}) and the image is bit-identical to n_devices = 1.  n = 0 removes the map
 * (logical = physical).  The environment variable RT_HIP_DEVICE_MAP="0,0,0", read at the first frame, sets the same map for
 * hosts that cannot call this (the reference's main.c behind libraytracer_amd.so).  Changing the map rebuilds the cached
 * context at the next frame.  Replaces nothing in the reference (its one parallel construct is the `omp parallel for` of
 * raytracer.c:184-185). */
int rt_hip_set_device_map(const int *map, int n);

/* The hierarchy builder of the scenes rt_hip_render_image() caches: RT_HIP_BVH_HOST (the default) or RT_HIP_BVH_DEVICE; another
 * value is RT_HIP_EINVAL.  Part of the cache key: a change rebuilds the cached context at the next frame. */
int rt_hip_set_bvh_builder(int builder);

/* on != 0: when a call's scene differs from the cached one ONLY in vertex positions, sphere centres and sphere radii -- the same
 * counts, flags, colours, emissions, tex coordinates, builder, devices and size -- every cached scene takes them in place
 * (rt_hip_scene_update_vertices_host, rt_hip_scene_update_spheres_host, both where both differ) and rt_hip_cache_updates() counts
 * one per frame, not rt_hip_cache_builds().  The default, 0: such a
 * scene rebuilds the context as any other change does. */
void rt_hip_set_scene_updates(int on);
uint64_t rt_hip_cache_updates(void);

/* on != 0: a call's scene may also differ from the cached one in flags, colours and emission (of spheres and meshes): every cached
 * scene takes them in place (rt_hip_scene_update_materials_host) and rt_hip_cache_updates() counts one per frame.  Independent of
 * rt_hip_set_scene_updates: a scene that differs both in materials and in positions is updated in place only if both switches
 * allow their part (still one count a frame); otherwise the context is rebuilt.  A device's chunk workspace, which is sized by the
 * scene's flag class, is freed by such an update and made again by the next chunked launch.  The default, 0: a changed material rebuilds the
 * context, whatever rt_hip_set_scene_updates says. */
void rt_hip_set_material_updates(int on);

/* The cached context's rebuild ratio: 0 (the default) never rebuilds; a finite ratio >= 1 makes every frame that
 * rt_hip_set_scene_updates(1) takes as an in-place VERTEX update end with rt_hip_scene_maintain_bvh(scene, ratio) on every cached
 * scene, and rt_hip_cache_rebuilds() counts the frames in which at least one of them rebuilt.  Another value (NaN, infinite,
 * negative, between 0 and 1) is RT_HIP_EINVAL and leaves the setting.  Not part of the cache key. */
int rt_hip_set_bvh_rebuild_ratio(double max_ratio);
uint64_t rt_hip_cache_rebuilds(void);

#ifdef __cplusplus
}
#endif

#endif /* RT_HIP_H */

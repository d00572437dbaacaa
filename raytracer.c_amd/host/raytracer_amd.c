/* raytracer_amd.c -- the reference's raytracer.h API on top of the HIP shim.
 *
 * This file is the host half of the drop-in: it exports every symbol the
 * reference's raytracer.o exports (reference
 * raytracer.h:135-164) with the same signatures and struct layouts, and
 * implements render() by handing the whole per-pixel loop nest
 * (reference raytracer.c:176-223) to librt_hip.so (include/rt_hip.h).
 *
 * The small host-side helpers (init_camera, intersect_sphere,
 * intersect_triangle, calculate_surface_normal, point_at) are the same
 * arithmetic, in the same order, as the device code, so a caller that probes
 * single primitives on the host sees what the GPU computes.
 *
 * No CPU rendering path: if the shim cannot run, render() says why on stderr
 * and exits with EXIT_FAILURE (the reference's own failure convention,
 * main.c:415-419; render() returns void, so there is no error channel).
 */
#include "raytracer.h"
#include "rt_hip.h"
#include "rt_rng.h"

long long ray_count = 0;
long long intersection_test_count = 0;

static int g_max_depth = MAX_DEPTH;
static uint64_t g_seed = 1666943821ull; /* reference main.c:182 */
static int g_devices = 0; /* 0: not set -- RT_DEVICES of the environment, else 1 (devices_to_use) */
static int g_integrator = RT_TRACE_PATH;
static uint64_t g_host_rng = 0;
static double g_last_seconds = 0;
static long long g_last_bounces = 0;
static int g_last_cancelled = 0;

_Static_assert(sizeof(Object) == sizeof(RtHipSphere), "Object must be passable as RtHipSphere");
_Static_assert(offsetof(Object, radius) == offsetof(RtHipSphere, radius), "Object.radius");
_Static_assert(offsetof(Object, center) == offsetof(RtHipSphere, center), "Object.center");
_Static_assert(offsetof(Object, color) == offsetof(RtHipSphere, color), "Object.color");
_Static_assert(offsetof(Object, emission) == offsetof(RtHipSphere, emission), "Object.emission");
_Static_assert(sizeof(Vertex) == sizeof(RtHipVertex), "Vertex must be passable as RtHipVertex");
_Static_assert(sizeof(Camera) == sizeof(RtHipCamera), "Camera must be passable as RtHipCamera");

/* ---- settings ------------------------------------------------------------------- */

void rt_set_max_depth(int max_depth) { g_max_depth = max_depth < 0 ? 0 : max_depth; }
int rt_get_max_depth(void) { return g_max_depth; }
void rt_set_seed(uint64_t seed)
{
  g_seed = seed;
  g_host_rng = 0;
}
uint64_t rt_get_seed(void) { return g_seed; }
void rt_set_devices(int n_devices) { g_devices = n_devices < 1 ? 1 : n_devices; }
void rt_set_integrator(int integrator)
{
  if (integrator == RT_TRACE_PATH || integrator == RT_CAST_RAY)
    g_integrator = integrator;
}
int rt_get_integrator(void) { return g_integrator; }

/* the thin lens of render() / render_ex(): stored as given, judged by the shim when a frame is rendered */
static double g_lens_aperture = 0.0, g_lens_focus = 1.0;
void rt_set_lens(double aperture_radius, double focus_distance)
{
  g_lens_aperture = aperture_radius;
  g_lens_focus = focus_distance;
}
void rt_get_lens(double *aperture_radius, double *focus_distance)
{
  if (aperture_radius)
    *aperture_radius = g_lens_aperture;
  if (focus_distance)
    *focus_distance = g_lens_focus;
}
/* the probe grid of render() / render_ex(): probes an axis; all 0: off */
static int g_probe_grid[3] = {0, 0, 0};
void rt_set_probe_grid(int nx, int ny, int nz)
{
  const int on = nx >= 1 && ny >= 1 && nz >= 1;
  g_probe_grid[0] = on ? nx : 0;
  g_probe_grid[1] = on ? ny : 0;
  g_probe_grid[2] = on ? nz : 0;
}
void rt_get_probe_grid(int *nx, int *ny, int *nz)
{
  if (nx)
    *nx = g_probe_grid[0];
  if (ny)
    *ny = g_probe_grid[1];
  if (nz)
    *nz = g_probe_grid[2];
}
/* the octahedral map's resolution of the probe grid's visibility weight; 0: off */
static int g_probe_vis_res = 0;
void rt_set_probe_visibility(int res) { g_probe_vis_res = res >= 2 && res <= 32 ? res : 0; }
int rt_get_probe_visibility(void) { return g_probe_vis_res; }
static int g_bvh_builder = RT_BVH_HOST;
void rt_set_bvh_builder(int builder)
{
  if ((builder == RT_BVH_HOST || builder == RT_BVH_DEVICE) && rt_hip_set_bvh_builder(builder) == RT_HIP_OK)
    g_bvh_builder = builder;
}
int rt_get_bvh_builder(void) { return g_bvh_builder; }
static int g_scene_updates = 0;
void rt_set_scene_updates(int on)
{
  g_scene_updates = on != 0;
  rt_hip_set_scene_updates(g_scene_updates);
}
int rt_get_scene_updates(void) { return g_scene_updates; }
static int g_material_updates = 0;
void rt_set_material_updates(int on)
{
  g_material_updates = on != 0;
  rt_hip_set_material_updates(g_material_updates);
}
int rt_get_material_updates(void) { return g_material_updates; }
static double g_bvh_rebuild_ratio = 0;
void rt_set_bvh_rebuild_ratio(double max_ratio)
{
  if (rt_hip_set_bvh_rebuild_ratio(max_ratio) == RT_HIP_OK)
    g_bvh_rebuild_ratio = max_ratio == 0 ? 0 : max_ratio;
}
double rt_get_bvh_rebuild_ratio(void) { return g_bvh_rebuild_ratio; }
double rt_last_render_seconds(void) { return g_last_seconds; }
static long long g_last_samples = 0; /* render_adaptive: pixel samples rendered */
static const volatile int *g_cancel_flag = NULL; /* render_progressive polls it between passes */
void rt_set_cancel_flag(const volatile int *flag)
{
  g_cancel_flag = flag;
  rt_hip_set_cancel_flag(flag);
}
int rt_last_render_cancelled(void) { return g_last_cancelled; }
long long rt_last_ray_bounces(void) { return g_last_bounces; }

/* ---- host-side RNG (reference raytracer.c:227-229) ------------------------------ */

/* The host stream is the (seed, pixel = 2^32-1, sample = 2^32-1) stream of
 * rt_rng.h: no image pixel can have that index (images are < 2^32 pixels). */
double random_double(void)
{
  if (!g_host_rng)
    g_host_rng = rt_rng_seed(g_seed, 0xFFFFFFFFu, 0xFFFFFFFFu);
  return rt_rng_double(&g_host_rng);
}

double random_range(double min, double max) { return random_double() * (max - min) + min; }

/* ---- primitives ----------------------------------------------------------------- */

vec3 point_at(const Ray *ray, double t)
{
  return vec3_add(ray->origin, vec3_scalar_mult(ray->direction, t));
}

/* Winding as the reference has it (raytracer.c:42-45): cross(v2-v0, v1-v0).
 * For (-1,1,1),(1,1,1),(1,1,-1) this is (0,-1,0) -- the reference's own
 * test.c:78 expects (0,1,0) and fails; the function, not the test, is the
 * behaviour every caller sees, so it is what is reproduced. */
vec3 calculate_surface_normal(vec3 v0, vec3 v1, vec3 v2)
{
  return vec3_normalize(vec3_cross(vec3_sub(v2, v0), vec3_sub(v1, v0)));
}

vec3 clamp(const vec3 v)
{
  vec3 r = {CLAMP(v.x), CLAMP(v.y), CLAMP(v.z)};
  return r;
}

/* reference raytracer.c:77-118 */
bool intersect_sphere(const Ray *ray, vec3 center, double radius, Hit *hit)
{
  intersection_test_count++;
  vec3 to_center = vec3_sub(center, ray->origin);
  double tca = vec3_dot(to_center, ray->direction);
  if (tca < 0)
    return false;
  double d2 = vec3_dot(to_center, to_center) - tca * tca;
  double r2 = radius * radius;
  if (d2 > r2)
    return false;
  double thc = sqrt(r2 - d2);
  double near_t = tca - thc, far_t = tca + thc;
  if (near_t > far_t)
  {
    double swap = near_t;
    near_t = far_t;
    far_t = swap;
  }
  if (near_t < 0)
    near_t = far_t; /* origin inside the sphere: leave through the far side */
  if (!(near_t > EPSILON))
    return false;
  hit->t = near_t;
  return true;
}

/* reference raytracer.c:120-174 */
bool intersect_triangle(const Ray *ray, Vertex vertex0, Vertex vertex1, Vertex vertex2, Hit *hit)
{
  intersection_test_count++;
  vec3 e1 = vec3_sub(vertex1.pos, vertex0.pos);
  vec3 e2 = vec3_sub(vertex2.pos, vertex0.pos);
  vec3 h = vec3_cross(ray->direction, e2);
  double det = vec3_dot(e1, h);
  if (det > -EPSILON && det < EPSILON)
    return false;
  double f = 1.0 / det;
  vec3 s = vec3_sub(ray->origin, vertex0.pos);
  double u = f * vec3_dot(s, h);
  if (u < 0.0 || u > 1.0)
    return false;
  vec3 q = vec3_cross(s, e1);
  double v = f * vec3_dot(ray->direction, q);
  if (v < 0.0 || u + v > 1.0)
    return false;
  double t = f * vec3_dot(e2, q);
  if (!(t > EPSILON))
    return false;
  vec2 tex = vec2_add(vec2_add(vec2_scalar_mult(vertex0.tex, 1 - u - v), vec2_scalar_mult(vertex1.tex, u)),
                      vec2_scalar_mult(vertex2.tex, v));
  hit->t = t;
  hit->u = tex.x;
  hit->v = tex.y;
  return true;
}

void print_v(const char *msg, const vec3 v) { printf("%s: (vec3) { %f, %f, %f }\n", msg, v.x, v.y, v.z); }

void print_m(const mat4 m)
{
  for (int r = 0; r < 4; r++)
  {
    for (int c = 0; c < 4; c++)
      printf(" %6.1f, ", m[r * 4 + c]);
    printf("\n");
  }
}

/* ---- camera (reference raytracer.c:47-75) ---------------------------------------- */

void init_camera(Camera *camera, vec3 position, vec3 target, Options *options)
{
  const double fov = 60.0 * (PI / 180); /* fixed 60 degree vertical field of view */
  const double half = tan(fov / 2);
  const double view_h = 2.0 * half;
  const double aspect = (double)options->width / (double)options->height;
  const double view_w = aspect * view_h;

  vec3 y_axis = {0, 1, 0};
  vec3 forward = vec3_normalize(vec3_sub(target, position));
  vec3 right = vec3_normalize(vec3_cross(y_axis, forward));
  vec3 up = vec3_normalize(vec3_cross(forward, right));

  camera->position = position;
  camera->vertical = vec3_scalar_mult(up, view_h);
  camera->horizontal = vec3_scalar_mult(right, view_w);
  vec3 half_v = vec3_scalar_div(camera->vertical, 2);
  vec3 half_h = vec3_scalar_div(camera->horizontal, 2);
  /* (pos - H/2) - (V/2 - (-forward)): with get_camera_ray's pos - (llc + Hu + Vv)
   * this yields an upright image with row 0 at the top. */
  camera->lower_left_corner =
      vec3_sub(vec3_sub(camera->position, half_h), vec3_sub(half_v, vec3_scalar_mult(forward, -1)));
}

/* ---- render ---------------------------------------------------------------------- */

/* rt_set_devices() wins; a host that never calls it (the reference's main.c, unmodified, behind this library) can be
 * given a device count through RT_DEVICES=N in the environment. */
static int devices_to_use(void)
{
  if (g_devices > 0)
    return g_devices;
  const char *e = getenv("RT_DEVICES");
  const int n = e ? atoi(e) : 0;
  return n >= 1 ? n : 1;
}

/* the shim's mesh records for the caller's MeshObjects (NULL for none; exits when out of memory, as render does) */
static RtHipMesh *hip_meshes(MeshObject *meshes, size_t n_meshes)
{
  RtHipMesh *hm = NULL;
  if (n_meshes)
  {
    hm = (RtHipMesh *)calloc(n_meshes, sizeof *hm);
    if (!hm)
    {
      fprintf(stderr, "render: out of memory\n");
      exit(EXIT_FAILURE);
    }
    for (size_t m = 0; m < n_meshes; m++)
    {
      hm[m].flags = meshes[m].flags;
      memcpy(hm[m].color, &meshes[m].color, sizeof hm[m].color);
      memcpy(hm[m].emission, &meshes[m].emission, sizeof hm[m].emission);
      hm[m].num_triangles = meshes[m].mesh.num_triangles;
      hm[m].vertices = (const RtHipVertex *)meshes[m].mesh.vertices;
    }
  }
  return hm;
}

/* the whole image, with the run-time settings */
static RtHipParams image_params(const Options *options)
{
  RtHipParams p;
  memset(&p, 0, sizeof p);
  p.width = options->width;
  p.height = options->height;
  p.samples = options->samples;
  p.max_depth = g_max_depth;
  p.seed = g_seed;
  p.integrator = g_integrator == RT_CAST_RAY ? RT_HIP_CAST_RAY : RT_HIP_TRACE_PATH;
  return p;
}

/* rt_set_probe_grid's grid for a scene: g_probe_grid probes an axis spanning [-reach, reach] about the world's origin, `reach` the
 * scene's own bound (rt_hip_scene_bounds: >= |p| for every point of a primitive of ordinary size; 1 where the scene has none); an axis
 * of one probe has it at 0.  origin = -reach, step = (2.0 * reach) / (double)(n - 1).  The bake's origin_radius is the cube's
 * corner, sqrt(3.0) * reach, a shade more. */
static int probe_grid_over(const RtHipScene *scene, RtHipProbeGrid *grid, RtHipProbeParams *pp)
{
  double reach = 0;
  const int rc = rt_hip_scene_bounds(scene, NULL, NULL, &reach, NULL);
  if (rc)
    return rc;
  if (!(reach > 0))
    reach = 1.0;
  rt_hip_probe_grid_defaults(grid);
  for (int a = 0; a < 3; a++)
  {
    const int n = g_probe_grid[a];
    grid->count[a] = (uint32_t)n;
    grid->origin[a] = n >= 2 ? -reach : 0.0;
    grid->step[a] = n >= 2 ? (2.0 * reach) / (double)(n - 1) : 1.0;
  }
  rt_hip_probe_defaults(pp);
  pp->origin_radius = sqrt(3.0) * reach * 1.0000001;
  return RT_HIP_OK;
}

/* ---- rt_set_probe_update: the scene and the grid's state that render_ex() keeps between calls -------------------------------------- */
static int g_probe_update_rays = 0;
static double g_probe_update_hysteresis = 0.9;
void rt_set_probe_update(int rays, double hysteresis)
{
  if (hysteresis >= 0 && hysteresis < 1)
    g_probe_update_hysteresis = hysteresis;
  g_probe_update_rays = rays > 0 ? rays : 0;
}
void rt_get_probe_update(int *rays, double *hysteresis)
{
  if (rays)
    *rays = g_probe_update_rays;
  if (hysteresis)
    *hysteresis = g_probe_update_hysteresis;
}

/* the scene of the previous call with deep copies of what it was made from, and the state of the grid derived from it */
static struct
{
  RtHipScene *scene;
  Object *objects;
  MeshObject *meshes; /* (each mesh.vertices is a copy of its own) */
  size_t n_objects, n_meshes;
  RtHipProbeGrid grid;
  int res, have_state;
  uint32_t round;
  double *coeff, *moments;
  uint32_t *age;
} g_kept;

static void kept_drop_state(void)
{
  free(g_kept.coeff);
  free(g_kept.moments);
  free(g_kept.age);
  g_kept.coeff = g_kept.moments = NULL;
  g_kept.age = NULL;
  g_kept.have_state = 0;
}

static void kept_drop(void)
{
  kept_drop_state();
  if (g_kept.scene)
    rt_hip_scene_destroy(g_kept.scene);
  for (size_t m = 0; m < g_kept.n_meshes; m++)
    free(g_kept.meshes[m].mesh.vertices);
  free(g_kept.meshes);
  free(g_kept.objects);
  memset(&g_kept, 0, sizeof g_kept);
}

/* does the call's scene equal the kept one but for sphere centres and radii and vertex positions -- and, under
 * rt_set_material_updates(1), flags, colours and emission (*recoloured says whether those differ)? */
static int kept_matches(const Object *objects, size_t n_objects, const MeshObject *meshes, size_t n_meshes, int *recoloured)
{
  *recoloured = 0;
  if (!g_kept.scene || n_objects != g_kept.n_objects || n_meshes != g_kept.n_meshes)
    return 0;
  for (size_t i = 0; i < n_objects; i++)
    if (objects[i].flags != g_kept.objects[i].flags || memcmp(&objects[i].color, &g_kept.objects[i].color, sizeof(vec3)) != 0 ||
        memcmp(&objects[i].emission, &g_kept.objects[i].emission, sizeof(vec3)) != 0)
      *recoloured = 1;
  for (size_t m = 0; m < n_meshes; m++)
  {
    const MeshObject *a = &meshes[m], *b = &g_kept.meshes[m];
    if (a->flags != b->flags || memcmp(&a->color, &b->color, sizeof(vec3)) != 0 || memcmp(&a->emission, &b->emission, sizeof(vec3)) != 0)
      *recoloured = 1;
    if ((*recoloured && !g_material_updates) || a->mesh.num_triangles != b->mesh.num_triangles)
      return 0;
    for (size_t k = 0; k < 3 * (size_t)a->mesh.num_triangles; k++)
      if (memcmp(&a->mesh.vertices[k].tex, &b->mesh.vertices[k].tex, sizeof(vec2)) != 0)
        return 0;
  }
  return !*recoloured || g_material_updates;
}

/* deep copies of the call's scene into g_kept (the scene handle apart); 0 when out of memory */
static int kept_copy(const Object *objects, size_t n_objects, const MeshObject *meshes, size_t n_meshes)
{
  g_kept.objects = (Object *)malloc(sizeof(Object) * (n_objects ? n_objects : 1));
  g_kept.meshes = (MeshObject *)calloc(n_meshes ? n_meshes : 1, sizeof(MeshObject));
  if (!g_kept.objects || !g_kept.meshes)
    return 0;
  memcpy(g_kept.objects, objects, sizeof(Object) * n_objects);
  g_kept.n_objects = n_objects;
  for (size_t m = 0; m < n_meshes; m++)
  {
    const size_t bytes = sizeof(Vertex) * 3 * (size_t)meshes[m].mesh.num_triangles;
    g_kept.meshes[m] = meshes[m];
    g_kept.meshes[m].mesh.vertices = (Vertex *)malloc(bytes ? bytes : 1);
    g_kept.n_meshes = m + 1;
    if (!g_kept.meshes[m].mesh.vertices)
      return 0;
    memcpy(g_kept.meshes[m].mesh.vertices, meshes[m].mesh.vertices, bytes);
  }
  return 1;
}

/* the kept scene takes the call's centres, radii and positions in place (rt_hip_scene_update_*_host) -- where they differ
 * (recoloured), its flags, colours and emission too (rt_hip_scene_update_materials_host) --, and so do the copies */
static int kept_take(const Object *objects, size_t n_objects, const MeshObject *meshes, size_t n_meshes, int recoloured)
{
  int rc = RT_HIP_OK;
  size_t n_tri = 0;
  for (size_t m = 0; m < n_meshes; m++)
    n_tri += (size_t)meshes[m].mesh.num_triangles;
  double *buf = (double *)malloc(sizeof(double) * (4 * n_objects + 9 * n_tri + 1));
  if (!buf)
    return RT_HIP_ENOMEM;
  if (n_objects)
  {
    for (size_t i = 0; i < n_objects; i++)
    {
      memcpy(buf + 4 * i, &objects[i].center, sizeof(vec3));
      buf[4 * i + 3] = objects[i].radius;
    }
    rc = rt_hip_scene_update_spheres_host(g_kept.scene, buf, n_objects);
  }
  if (!rc && n_tri)
  {
    double *pos = buf + 4 * n_objects;
    size_t at = 0;
    for (size_t m = 0; m < n_meshes; m++)
      for (size_t k = 0; k < 3 * (size_t)meshes[m].mesh.num_triangles; k++, at += 3)
        memcpy(pos + at, &meshes[m].mesh.vertices[k].pos, sizeof(vec3));
    rc = rt_hip_scene_update_vertices_host(g_kept.scene, pos, n_tri);
  }
  free(buf);
  if (!rc && recoloured)
  {
    const size_t n = n_objects + n_meshes;
    double *mat = (double *)malloc(sizeof(double) * 6 * n);
    uint32_t *flags = (uint32_t *)malloc(sizeof(uint32_t) * n);
    rc = mat && flags ? RT_HIP_OK : RT_HIP_ENOMEM;
    for (size_t i = 0; !rc && i < n; i++)
    {
      memcpy(mat + 6 * i, i < n_objects ? &objects[i].color : &meshes[i - n_objects].color, sizeof(vec3));
      memcpy(mat + 6 * i + 3, i < n_objects ? &objects[i].emission : &meshes[i - n_objects].emission, sizeof(vec3));
      flags[i] = i < n_objects ? objects[i].flags : meshes[i - n_objects].flags;
    }
    if (!rc)
      rc = rt_hip_scene_update_materials_host(g_kept.scene, mat, flags, n);
    free(mat);
    free(flags);
  }
  if (!rc)
  {
    memcpy(g_kept.objects, objects, sizeof(Object) * n_objects);
    for (size_t m = 0; m < n_meshes; m++)
    {
      g_kept.meshes[m].flags = meshes[m].flags;
      g_kept.meshes[m].color = meshes[m].color;
      g_kept.meshes[m].emission = meshes[m].emission;
    }
    for (size_t m = 0; m < n_meshes; m++)
      memcpy(g_kept.meshes[m].mesh.vertices, meshes[m].mesh.vertices, sizeof(Vertex) * 3 * (size_t)meshes[m].mesh.num_triangles);
  }
  return rc;
}

/* render_ex()'s probe-lit frame under rt_set_probe_update: the kept scene where the call's scene matches it, else a new one that is
 * kept; one round and the preview where the derived grid is the previous call's too, else the full bake, whose state is kept */
static int render_probe_following(uint8_t *framebuffer, float *linear_rgb, Object *objects, size_t n_objects, MeshObject *meshes,
                                  size_t n_meshes, const RtHipMesh *hm, Camera *camera, const RtHipParams *p, uint64_t *stats)
{
  int recoloured = 0;
  int rc, same_scene = kept_matches(objects, n_objects, meshes, n_meshes, &recoloured);
  if (same_scene && kept_take(objects, n_objects, meshes, n_meshes, recoloured) != RT_HIP_OK)
    same_scene = 0; /* (an update the scene refuses: start over) */
  if (!same_scene)
  {
    kept_drop();
    rc = rt_hip_scene_create((const RtHipSphere *)objects, n_objects, hm, n_meshes, 0, &g_kept.scene);
    if (rc)
      return rc;
    if (!kept_copy(objects, n_objects, meshes, n_meshes))
    {
      kept_drop();
      return RT_HIP_ENOMEM;
    }
  }
  RtHipProbeGrid grid;
  RtHipProbeParams pp;
  RtHipProbeVis vis;
  rc = probe_grid_over(g_kept.scene, &grid, &pp);
  if (rc)
    return rc;
  pp.max_depth = p->max_depth;
  pp.seed = p->seed;
  rt_hip_probe_vis_defaults(&vis, &grid);
  vis.res = (uint32_t)(g_probe_vis_res > 0 ? g_probe_vis_res : 2);
  const RtHipProbeVis *v = g_probe_vis_res > 0 ? &vis : NULL;
  if (same_scene && g_kept.have_state && g_kept.res == g_probe_vis_res &&
      memcmp(grid.count, g_kept.grid.count, sizeof grid.count) == 0 && memcmp(grid.origin, g_kept.grid.origin, sizeof grid.origin) == 0 &&
      memcmp(grid.step, g_kept.grid.step, sizeof grid.step) == 0) /* (the same counts and the same reach) */
  {
    RtHipProbeUpdate upd;
    rt_hip_probe_update_defaults(&upd);
    upd.hysteresis = g_probe_update_hysteresis;
    upd.round = ++g_kept.round;
    pp.samples = g_probe_update_rays;
    rc = rt_hip_probe_update_preview_scene_image(g_kept.scene, (const RtHipCamera *)camera, &grid, v, &pp, &upd, p->width, p->height, 1,
                                                 linear_rgb, framebuffer, g_kept.coeff, v ? g_kept.moments : NULL, g_kept.age, stats);
    if (rc)
      kept_drop();
    return rc;
  }
  kept_drop_state();
  const size_t n = (size_t)grid.count[0] * grid.count[1] * grid.count[2], texels = (size_t)vis.res * vis.res;
  g_kept.coeff = (double *)malloc(sizeof(double) * 27 * n);
  g_kept.moments = (double *)malloc(sizeof(double) * 2 * texels * n);
  g_kept.age = (uint32_t *)malloc(sizeof(uint32_t) * n);
  if (!g_kept.coeff || !g_kept.moments || !g_kept.age)
  {
    kept_drop();
    return RT_HIP_ENOMEM;
  }
  pp.samples = p->samples;
  if (v)
    rc = rt_hip_probe_preview_vis_scene_image(g_kept.scene, (const RtHipCamera *)camera, &grid, v, &pp, p->width, p->height, 1, linear_rgb,
                                              framebuffer, g_kept.coeff, g_kept.moments, stats);
  else
    rc = rt_hip_probe_preview_scene_image(g_kept.scene, (const RtHipCamera *)camera, &grid, &pp, p->width, p->height, 1, linear_rgb, framebuffer,
                                          g_kept.coeff, stats);
  if (rc)
  {
    kept_drop();
    return rc;
  }
  for (size_t i = 0; i < n; i++)
    g_kept.age[i] = 1u; /* the bake stands for one round */
  g_kept.grid = grid;
  g_kept.res = g_probe_vis_res;
  g_kept.round = 0;
  g_kept.have_state = 1;
  return RT_HIP_OK;
}

void render_ex(uint8_t *framebuffer, float *linear_rgb, Object *objects, size_t n_objects,
               MeshObject *meshes, size_t n_meshes, Camera *camera, Options *options)
{
  RtHipMesh *hm = hip_meshes(meshes, n_meshes);
  RtHipParams p = image_params(options);

  uint64_t stats[RT_HIP_NSTATS] = {0, 0, 0, 0};
  double seconds = 0;
  int rc;
  const int following = g_probe_grid[0] > 0 && g_probe_update_rays > 0 && g_scene_updates;
  if (!following)
    kept_drop(); /* (a frame of any other kind keeps nothing) */
  if (following)
  { /* the probe-lit preview with the scene and the grid's state kept between calls (rt_set_probe_update) */
    struct timespec t0, t1;
    clock_gettime(CLOCK_MONOTONIC, &t0);
    rc = render_probe_following(framebuffer, linear_rgb, objects, n_objects, meshes, n_meshes, hm, camera, &p, stats);
    clock_gettime(CLOCK_MONOTONIC, &t1);
    seconds = (double)(t1.tv_sec - t0.tv_sec) + 1e-9 * (double)(t1.tv_nsec - t0.tv_nsec);
  }
  else if (g_probe_grid[0] > 0)
  { /* the probe-lit preview on ONE scene: a grid over its bounds, options->samples rays a probe, one first-hit sample a pixel */
    RtHipScene *scene = NULL;
    RtHipProbeGrid grid;
    RtHipProbeParams pp;
    struct timespec t0, t1;
    clock_gettime(CLOCK_MONOTONIC, &t0);
    rc = rt_hip_scene_create((const RtHipSphere *)objects, n_objects, hm, n_meshes, 0, &scene);
    if (!rc)
      rc = probe_grid_over(scene, &grid, &pp);
    if (!rc)
    {
      pp.samples = p.samples;
      pp.max_depth = p.max_depth;
      pp.seed = p.seed;
      if (g_probe_vis_res > 0)
      { /* ... with every corner weighed by its baked visibility: the defaults for this grid at the chosen resolution */
        RtHipProbeVis vis;
        rt_hip_probe_vis_defaults(&vis, &grid);
        vis.res = (uint32_t)g_probe_vis_res;
        rc = rt_hip_probe_preview_vis_scene_image(scene, (const RtHipCamera *)camera, &grid, &vis, &pp, p.width, p.height, 1, linear_rgb,
                                                  framebuffer, NULL, NULL, stats);
      }
      else
        rc = rt_hip_probe_preview_scene_image(scene, (const RtHipCamera *)camera, &grid, &pp, p.width, p.height, 1, linear_rgb, framebuffer,
                                              NULL, stats);
    }
    if (scene)
      rt_hip_scene_destroy(scene);
    clock_gettime(CLOCK_MONOTONIC, &t1);
    seconds = (double)(t1.tv_sec - t0.tv_sec) + 1e-9 * (double)(t1.tv_nsec - t0.tv_nsec);
  }
  else if (g_lens_aperture > 0)
  { /* depth of field: the lens frame, on one device; the seconds are the call's, by the host's clock */
    RtHipLens lens;
    rt_hip_lens_defaults(&lens);
    lens.aperture_radius = g_lens_aperture;
    lens.focus_distance = g_lens_focus;
    struct timespec t0, t1;
    clock_gettime(CLOCK_MONOTONIC, &t0);
    rc = rt_hip_render_lens_image((const RtHipSphere *)objects, n_objects, hm, n_meshes, (const RtHipCamera *)camera, &lens, &p, 0,
                                  linear_rgb, framebuffer, stats);
    clock_gettime(CLOCK_MONOTONIC, &t1);
    seconds = (double)(t1.tv_sec - t0.tv_sec) + 1e-9 * (double)(t1.tv_nsec - t0.tv_nsec);
  }
  else
    rc = rt_hip_render_image((const RtHipSphere *)objects, n_objects, hm, n_meshes, (const RtHipCamera *)camera,
                             &p, devices_to_use(), linear_rgb, framebuffer, stats, &seconds);
  free(hm);
  g_last_cancelled = rc == RT_HIP_ECANCELLED;
  if (rc != RT_HIP_OK && rc != RT_HIP_ECANCELLED)
  {
    fprintf(stderr, "render: GPU path failed (%d): %s\n", rc, rt_hip_last_error());
    exit(EXIT_FAILURE);
  }
  /* the reference's globals accumulate over calls (raytracer.c:36-37, 79, 484) */
  ray_count += (long long)stats[RT_HIP_STAT_RAYS];
  intersection_test_count += (long long)stats[RT_HIP_STAT_TESTS];
  g_last_seconds = seconds;
  g_last_bounces = (long long)stats[RT_HIP_STAT_CASTS];
}

void render(uint8_t *framebuffer, Object *objects, size_t n_objects, Camera *camera, Options *options)
{
  render_ex(framebuffer, NULL, objects, n_objects, NULL, 0, camera, options);
}

int render_progressive(uint8_t *framebuffer, float *linear_rgb, Object *objects, size_t n_objects, MeshObject *meshes,
                       size_t n_meshes, Camera *camera, Options *options, int pass_samples, RtPassFn *on_pass, void *user)
{
  if (devices_to_use() > 1)
  {
    fprintf(stderr, "render_progressive: renders on one device (%d set)\n", devices_to_use());
    return RT_HIP_EINVAL;
  }
  if (pass_samples < 1)
  {
    fprintf(stderr, "render_progressive: pass_samples must be >= 1\n");
    return RT_HIP_EINVAL;
  }
  RtHipMesh *hm = hip_meshes(meshes, n_meshes);
  RtHipParams p = image_params(options);
  p.tile_first = 0;
  p.tile_stride = 1;
  p.tile_count = (uint32_t)(((options->width + RT_HIP_TILE - 1) / RT_HIP_TILE) * ((options->height + RT_HIP_TILE - 1) / RT_HIP_TILE));
  RtHipScene *scene = NULL;
  RtHipAccum *acc = NULL;
  uint64_t stats[RT_HIP_NSTATS] = {0, 0, 0, 0};
  double seconds = 0;
  int done = 0;
  int rc = rt_hip_scene_create((const RtHipSphere *)objects, n_objects, hm, n_meshes, 0, &scene);
  if (!rc)
    rc = rt_hip_accum_create(scene, (const RtHipCamera *)camera, &p, &acc);
  while (!rc)
  {
    const int n = pass_samples < p.samples - done ? pass_samples : p.samples - done;
    double pass_s = 0;
    rc = rt_hip_accum_add_host(acc, n, stats, &pass_s);
    if (rc)
      break;
    done += n;
    seconds += pass_s;
    if (on_pass)
      on_pass(done, p.samples, pass_s, user);
    if (done >= p.samples || (g_cancel_flag && *g_cancel_flag))
      break;
  }
  if (!rc)
    rc = rt_hip_accum_read_image(acc, linear_rgb, framebuffer);
  if (rc)
    fprintf(stderr, "render_progressive: GPU path failed (%d): %s\n", rc, rt_hip_last_error());
  rt_hip_accum_destroy(acc);
  rt_hip_scene_destroy(scene);
  free(hm);
  if (rc)
    return rc;
  g_last_cancelled = done < p.samples;
  ray_count += (long long)stats[RT_HIP_STAT_RAYS];
  intersection_test_count += (long long)stats[RT_HIP_STAT_TESTS];
  g_last_seconds = seconds;
  g_last_bounces = (long long)stats[RT_HIP_STAT_CASTS];
  return done;
}

typedef struct
{
  RtCheckpointFn *fn;
  void *user;
  int total, done;
} AdaptHook;

static int adapt_checkpoint(void *user, int32_t done, uint32_t live)
{
  AdaptHook *h = (AdaptHook *)user;
  h->done = done;
  if (h->fn)
    h->fn(done, h->total, live, h->user);
  return g_cancel_flag && *g_cancel_flag;
}

int render_adaptive(uint8_t *framebuffer, float *linear_rgb, uint32_t *tile_samples, Object *objects, size_t n_objects,
                    MeshObject *meshes, size_t n_meshes, Camera *camera, Options *options, const RtHipAdaptParams *params,
                    RtCheckpointFn *on_checkpoint, void *user)
{
  if (devices_to_use() > 1)
  {
    fprintf(stderr, "render_adaptive: renders on one device (%d set)\n", devices_to_use());
    return RT_HIP_EINVAL;
  }
  if (!camera || !options || (!framebuffer && !linear_rgb))
  {
    fprintf(stderr, "render_adaptive: camera, options and an output are required\n");
    return RT_HIP_EINVAL;
  }
  RtHipMesh *hm = hip_meshes(meshes, n_meshes);
  RtHipParams p = image_params(options);
  const size_t n_tiles = (size_t)((options->width + RT_HIP_TILE - 1) / RT_HIP_TILE) * (size_t)((options->height + RT_HIP_TILE - 1) / RT_HIP_TILE);
  uint32_t *counts = tile_samples ? tile_samples : (uint32_t *)calloc(n_tiles ? n_tiles : 1, sizeof(uint32_t));
  uint64_t stats[RT_HIP_NSTATS] = {0, 0, 0, 0};
  double seconds = 0;
  AdaptHook hook = {on_checkpoint, user, p.samples, 0};
  int rc = counts ? rt_hip_render_adaptive_image((const RtHipSphere *)objects, n_objects, hm, n_meshes, (const RtHipCamera *)camera, &p, params,
                                                 0, linear_rgb, framebuffer, counts, stats, &seconds, adapt_checkpoint, &hook)
                  : RT_HIP_ENOMEM;
  free(hm);
  const int cancelled = rc == RT_HIP_ECANCELLED;
  int most = 0;
  if (!rc || cancelled)
    for (size_t k = 0; k < n_tiles; k++)
      most = (int)counts[k] > most ? (int)counts[k] : most;
  if (counts != tile_samples)
    free(counts);
  if (rc && !cancelled)
  {
    fprintf(stderr, "render_adaptive: GPU path failed (%d): %s\n", rc, rc == RT_HIP_ENOMEM && !counts ? "out of host memory" : rt_hip_last_error());
    return rc;
  }
  g_last_cancelled = cancelled;
  ray_count += (long long)stats[RT_HIP_STAT_RAYS];
  intersection_test_count += (long long)stats[RT_HIP_STAT_TESTS];
  g_last_seconds = seconds;
  g_last_bounces = (long long)stats[RT_HIP_STAT_CASTS];
  g_last_samples = (long long)stats[RT_HIP_STAT_SAMPLES];
  return most;
}

long long rt_last_pixel_samples(void) { return g_last_samples; }

int render_aov(RtAovImage *out, Object *objects, size_t n_objects, MeshObject *meshes, size_t n_meshes, Camera *camera,
               Options *options)
{
  if (!out || !camera || !options)
  {
    fprintf(stderr, "render_aov: out, camera and options are required\n");
    return RT_HIP_EINVAL;
  }
  RtHipMesh *hm = hip_meshes(meshes, n_meshes);
  RtHipParams p = image_params(options);
  const RtHipAov h = {out->albedo, out->normal, out->depth, out->object_id, out->hits};
  const int rc = rt_hip_render_aov_image((const RtHipSphere *)objects, n_objects, hm, n_meshes, (const RtHipCamera *)camera, &p, 0, &h);
  free(hm);
  if (rc)
  {
    fprintf(stderr, "render_aov: GPU path failed (%d): %s\n", rc, rt_hip_last_error());
    return rc;
  }
  return p.samples;
}

int denoise_frame(uint8_t *framebuffer, float *linear_out, const float *linear_in, const RtAovImage *aov, int width, int height,
                  const RtHipDenoiseParams *params)
{
  RtHipDenoiseParams defaults;
  rt_hip_denoise_defaults(&defaults);
  if (!aov)
  {
    fprintf(stderr, "denoise_frame: the feature buffers are required\n");
    return RT_HIP_EINVAL;
  }
  const RtHipAov h = {aov->albedo, aov->normal, aov->depth, aov->object_id, aov->hits};
  const int rc = rt_hip_denoise_image(linear_in, &h, width, height, params ? params : &defaults, 0, linear_out, framebuffer);
  if (rc)
    fprintf(stderr, "denoise_frame: GPU path failed (%d): %s\n", rc, rt_hip_last_error());
  return rc;
}

int reproject_frame(uint8_t *framebuffer, float *linear_out, float *len_out, float *motion_out, const float *linear_in,
                    const RtAovImage *aov, const Camera *camera, const float *hist_linear, const float *hist_len,
                    const RtAovImage *hist_aov, const Camera *hist_camera, int width, int height, const RtHipReprojectParams *params)
{
  RtHipReprojectParams defaults;
  rt_hip_reproject_defaults(&defaults);
  if (!aov)
  {
    fprintf(stderr, "reproject_frame: the feature buffers are required\n");
    return RT_HIP_EINVAL;
  }
  const RtHipAov h = {aov->albedo, aov->normal, aov->depth, aov->object_id, aov->hits};
  RtHipAov hh = {NULL, NULL, NULL, NULL, NULL};
  if (hist_aov)
  {
    const RtHipAov given = {hist_aov->albedo, hist_aov->normal, hist_aov->depth, hist_aov->object_id, hist_aov->hits};
    hh = given;
  }
  const int rc = rt_hip_reproject_image(linear_in, &h, (const RtHipCamera *)camera, hist_linear, hist_len, hist_aov ? &hh : NULL,
                                        (const RtHipCamera *)hist_camera, width, height, params ? params : &defaults, 0, linear_out,
                                        framebuffer, len_out, motion_out);
  if (rc)
    fprintf(stderr, "reproject_frame: GPU path failed (%d): %s\n", rc, rt_hip_last_error());
  return rc;
}

int upsample_frame(uint8_t *framebuffer, float *linear_out, float *conf_out, const float *linear_low, const RtAovImage *aov_low,
                   int low_width, int low_height, const RtAovImage *aov, int width, int height, const RtHipUpsampleParams *params)
{
  RtHipUpsampleParams defaults;
  rt_hip_upsample_defaults(&defaults);
  if (!aov_low || !aov)
  {
    fprintf(stderr, "upsample_frame: the feature buffers of both frames are required\n");
    return RT_HIP_EINVAL;
  }
  const size_t n = width > 0 && height > 0 ? (size_t)width * (size_t)height : 0;
  float *own = linear_out ? NULL : (float *)malloc((n ? n : 1) * 3 * sizeof(float)); /* the shim's out_rgb is required */
  if (!linear_out && !own)
  {
    fprintf(stderr, "upsample_frame: could not allocate the linear frame\n");
    return RT_HIP_ENOMEM;
  }
  const RtHipAov l = {aov_low->albedo, aov_low->normal, aov_low->depth, aov_low->object_id, aov_low->hits};
  const RtHipAov h = {aov->albedo, aov->normal, aov->depth, aov->object_id, aov->hits};
  const int rc = rt_hip_upsample_image(linear_low, &l, low_width, low_height, &h, width, height, params ? params : &defaults, 0,
                                       linear_out ? linear_out : own, framebuffer, conf_out);
  free(own);
  if (rc)
    fprintf(stderr, "upsample_frame: GPU path failed (%d): %s\n", rc, rt_hip_last_error());
  return rc;
}

int intersect_rays(const Ray *rays, size_t n, const double *t_max, Object *objects, size_t n_objects, MeshObject *meshes,
                   size_t n_meshes, Hit *hits, uint8_t *status)
{
  if (!hits || (n && !rays))
  {
    fprintf(stderr, "intersect_rays: rays and hits are required\n");
    return RT_HIP_EINVAL;
  }
  if (n == 0)
    return 0;
  /* one block: status, object, prim (words), then t, point, normal, bary (doubles) */
  uint32_t *words = (uint32_t *)malloc(n * (3 * sizeof(uint32_t) + 9 * sizeof(double)) + sizeof(double));
  if (!words)
  {
    fprintf(stderr, "intersect_rays: out of memory\n");
    return RT_HIP_ENOMEM;
  }
  uint32_t *st = words, *object = words + n, *prim = words + 2 * n;
  double *t = (double *)(((uintptr_t)(words + 3 * n) + 7u) & ~(uintptr_t)7u), *point = t + n, *normal = point + 3 * n, *bary = normal + 3 * n;
  RtHipMesh *hm = hip_meshes(meshes, n_meshes);
  RtHipQueryParams p;
  rt_hip_query_defaults(&p);
  const RtHipHits h = {st, t, object, prim, point, normal, bary, NULL};
  const int rc = rt_hip_query_rays_host((const RtHipSphere *)objects, n_objects, hm, n_meshes, (const double *)rays, t_max, n, &p, 0, &h);
  free(hm);
  if (rc)
  {
    fprintf(stderr, "intersect_rays: GPU path failed (%d): %s\n", rc, rt_hip_last_error());
    free(words);
    return rc;
  }
  for (size_t i = 0; i < n; i++)
  {
    Hit out;
    memset(&out, 0, sizeof out);
    out.t = DBL_MAX;
    out.object_id = 0xFFFFFFFFu;
    if (st[i] == 1u)
    {
      out.t = t[i];
      out.point = (vec3){point[3 * i], point[3 * i + 1], point[3 * i + 2]};
      out.normal = (vec3){normal[3 * i], normal[3 * i + 1], normal[3 * i + 2]};
      out.object_id = object[i];
      if (prim[i] == 0xFFFFFFFFu)
      { /* raytracer.c:410-411 */
        out.u = atan2(out.normal.x, out.normal.z) / (2 * PI) + 0.5;
        out.v = out.normal.y * 0.5 + 0.5;
      }
      else
      { /* the winner's triangle: prim counts through the meshes in array order; raytracer.c:154-167 */
        size_t k = prim[i], m = 0;
        while (m < n_meshes && k >= meshes[m].mesh.num_triangles)
          k -= meshes[m++].mesh.num_triangles;
        if (m < n_meshes)
        {
          const Vertex *v = meshes[m].mesh.vertices + 3 * k;
          const double bu = bary[2 * i], bv = bary[2 * i + 1];
          const vec2 tex = vec2_add(vec2_add(vec2_scalar_mult(v[0].tex, 1 - bu - bv), vec2_scalar_mult(v[1].tex, bu)),
                                    vec2_scalar_mult(v[2].tex, bv));
          out.u = tex.x;
          out.v = tex.y;
        }
      }
    }
    hits[i] = out;
    if (status)
      status[i] = (uint8_t)st[i];
  }
  free(words);
  return 0;
}

int trace_rays(const Ray *rays, size_t n, int samples, Object *objects, size_t n_objects, MeshObject *meshes, size_t n_meshes,
               vec3 *radiance, uint8_t *status)
{
  if (!radiance || (n && !rays))
  {
    fprintf(stderr, "trace_rays: rays and radiance are required\n");
    return RT_HIP_EINVAL;
  }
  if (n == 0)
    return 0;
  uint32_t *st = (uint32_t *)malloc(n * sizeof(uint32_t));
  if (!st)
  {
    fprintf(stderr, "trace_rays: out of memory\n");
    return RT_HIP_ENOMEM;
  }
  RtHipMesh *hm = hip_meshes(meshes, n_meshes);
  RtHipTraceParams p;
  rt_hip_trace_defaults(&p);
  p.samples = samples;
  p.max_depth = g_max_depth;
  p.seed = g_seed;
  const RtHipRadiance out = {st, (double *)radiance, NULL, NULL, NULL, NULL}; /* vec3: three doubles */
  uint64_t stats[RT_HIP_NSTATS] = {0, 0, 0, 0};
  const int rc = rt_hip_trace_rays_host((const RtHipSphere *)objects, n_objects, hm, n_meshes, (const double *)rays, n, &p, 0, &out, stats);
  free(hm);
  if (rc)
    fprintf(stderr, "trace_rays: GPU path failed (%d): %s\n", rc, rt_hip_last_error());
  else
  {
    ray_count += (long long)stats[0];
    intersection_test_count += (long long)stats[2];
    for (size_t i = 0; status && i < n; i++)
      status[i] = (uint8_t)st[i];
  }
  free(st);
  return rc;
}

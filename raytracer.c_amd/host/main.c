/* main.c -- command-line host, the counterpart of the reference's main.c.
 *
 * Same flags (-w -h -s -o, reference main.c:149-174; note -h is HEIGHT there
 * too) and the same default scene (the 38-sphere room, main.c:244-397, camera
 * main.c:425, seed main.c:182), through the same API calls a reference caller
 * makes: init_camera(), render(), stbi_write_png().  Extra flags select what
 * the reference fixes at compile time:
 *   -d <depth>   bounce limit (reference MAX_DEPTH, raytracer.h:25; default 5)
 *   -c <config>  scene 1..5 of BASELINE.json (default 4, the reference's room)
 *   -g <gpus>    GPUs of this node to spread the image over (default 1)
 *   -r <seed>    RNG seed (default 1666943821)
 *   -i <0|1>     integrator: 0 trace_path (default), 1 cast_ray -- the `#if 1` of
 *                raytracer.c:207-211
 *   -b <0|1>     who builds the triangle hierarchy: 0 the host (default), 1 the device (rt_set_bvh_builder): the same
 *                PNG either way, only the scene's build time differs
 *   -p <samples> progressive: add the samples in passes of this many (render_progressive, one GPU), a
 *                line per pass; the PNG is the one-shot image bit for bit
 *   -a <prefix>  after the frame, its first-hit feature buffers (render_aov: the frame's own camera samples, same -s
 *                and seed, one GPU): <prefix>_albedo.pfm and <prefix>_normal.pfm (PF, 3 channels), <prefix>_depth.pfm
 *                (Pf) -- little-endian, rows stored bottom to top as PFM has them, so they show the PNG's picture
 *   -n <iters>   denoise (denoise_frame, rt_hip_denoise's defaults with this many iterations, 0..10, one GPU): after the
 *                frame, the first-hit buffers of its own samples (as -a; with -p the samples done), then the denoised PNG to
 *                -o and the frame as rendered to <name>.noisy.png (-o's name without .png)
 *   -q <x,y>     query instead of rendering: what the ray through the centre of pixel (x, y) of the chosen scene and size hits
 *                (rt_hip_query_rays_host with u = (x + 0.5) / (w - 1), v = (y + 0.5) / (h - 1)): status, object id,
 *                primitive, t, point and normal, one line each.  Nothing is rendered or written.
 *   -k <x,y,z>   a light probe instead of rendering: the 27 SH9 radiance coefficients of the chosen scene at that point
 *                (rt_hip_bake_probes_host, RT_HIP_PROBE_SPHERE, -s rays, -d and -r as given): status and nine lines of three
 *                channels.  Nothing is rendered or written.
 *   -m <nx,ny,nz[,res]> the probe-lit preview in the frame's place (rt_set_probe_grid): a grid of nx x ny x nz light probes over the
 *                scene's bounds, -s rays a probe, -d and -r as given; the PNG is rt_hip_probe_preview_image's frame.  One GPU.  A fourth
 *                number, 2 .. 32, weighs every probe by its baked visibility (rt_set_probe_visibility): depth moments in res x res maps.
 *   -u <f>       preview by guided upsampling, integer f >= 2 (upsample_frame, rt_hip_upsample's defaults, one GPU): the frame is
 *                rendered at ceil(w / f) x ceil(h / f) under the full size's camera (with -n: and denoised there), the first-hit
 *                buffers are rendered at both sizes, and the low frame is brought to w x h under the full-size buffers.  The PNG
 *                goes to -o, the low frame to <name>.low.png.  Not with -g > 1, -e, -q, -p or -a.
 * Timing is wall-clock (the reference's clock()/integer division, main.c:427-433,
 * reports summed CPU time truncated to seconds -- deliberately not reproduced).
 * SIGINT: the reference's handler writes and frees the live framebuffer from
 * signal context (main.c:37-48); here it only sets a flag that the renderer
 * polls between slabs of tiles, and the partial image is written normally.
 * With -p it is polled between passes, and the image is whole, of fewer samples.
 */
#define _POSIX_C_SOURCE 200809L
#include <signal.h>
#include <time.h>

#include "raytracer.h"
#include "rt_hip.h"
#include "scenes.h"

int stbi_write_png(char const *filename, int w, int h, int comp, const void *data, int stride_in_bytes);

static volatile int interrupted = 0; /* polled by the renderer between slabs of tiles */
static void on_sigint(int sig)
{
  (void)sig;
  interrupted = 1;
}

/* -p: one line per pass */
static void on_checkpoint(int done, int total, unsigned live_tiles, void *user)
{
  (void)user;
  printf("checkpoint: %d of %d samples, %u tiles live\n", done, total, live_tiles);
  fflush(stdout);
}

static void on_pass(int done, int total, double kernel_seconds, void *user)
{
  (void)user;
  printf("pass: %d / %d samples per pixel (GPU kernels %f s)\n", done, total, kernel_seconds);
  fflush(stdout);
}

/* -a: one PFM file, little-endian (scale -1.0), rows bottom to top; `rows` is row-major with row 0 at the top (as the PNG) */
static int write_pfm(const char *prefix, const char *name, const float *rows, int w, int h, int channels)
{
  char path[4096];
  if (snprintf(path, sizeof path, "%s_%s.pfm", prefix, name) >= (int)sizeof path)
    return -1;
  FILE *f = fopen(path, "wb");
  if (!f)
    return -1;
  int ok = fprintf(f, "%s\n%d %d\n-1.0\n", channels == 3 ? "PF" : "Pf", w, h) > 0;
  const size_t row_vals = (size_t)w * channels;
  uint8_t *buf = (uint8_t *)malloc(row_vals * 4);
  ok = ok && buf;
  for (int y = h - 1; ok && y >= 0; y--)
  {
    for (size_t k = 0; k < row_vals; k++)
    {
      uint32_t u;
      memcpy(&u, &rows[(size_t)y * row_vals + k], 4);
      buf[4 * k + 0] = (uint8_t)u;
      buf[4 * k + 1] = (uint8_t)(u >> 8);
      buf[4 * k + 2] = (uint8_t)(u >> 16);
      buf[4 * k + 3] = (uint8_t)(u >> 24);
    }
    ok = fwrite(buf, 4, row_vals, f) == row_vals;
  }
  free(buf);
  ok = (fclose(f) == 0) && ok;
  if (ok)
    printf("wrote '%s'\n", path);
  return ok ? 0 : -1;
}

static double now_seconds(void)
{
  struct timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}

typedef struct
{
  Options options;
  int depth, config, gpus, integrator;
  int bvh;  /* -b: RT_BVH_HOST or RT_BVH_DEVICE */
  int pass; /* -p: samples per pass; 0: not given (one-shot) */
  const char *aov; /* -a: prefix of the feature-buffer files; NULL: none */
  int denoise;     /* -n: iterations + 1; 0: not given */
  int adaptive;    /* -e given */
  double threshold; /* -e: the error at or below which a tile stops */
  int upsample;     /* -u: the factor; 0: not given */
  int query;        /* -q given */
  double qx, qy;    /* -q: the pixel */
  int lens;         /* -l given */
  double lens_aperture, lens_focus; /* -l: the thin lens' aperture radius and focus distance */
  int probe;        /* -k given */
  double probe_at[3]; /* -k: the light probe's position */
  int grid[3];      /* -m: probes an axis of the probe-lit preview; 0: not given */
  int grid_vis;     /* -m's fourth number: the resolution of the probes' visibility maps; 0: not given */
  uint64_t seed;
} Args;

static void usage(const char *prog)
{
  fprintf(stderr,
          "Usage: %s -w <width> -h <height> -s <samples per pixel> -o <filename>\n"
          "          [-d <max depth>] [-c <scene config 1..5>] [-g <gpus>] [-r <seed>]\n"
          "          [-i <integrator: 0 trace_path, 1 cast_ray>] [-p <samples per pass, one GPU>]\n"
          "          [-b <triangle hierarchy built by: 0 the host, 1 the device>]\n"
          "          [-a <prefix of the albedo / normal / depth .pfm files>]\n"
          "          [-n <denoise iterations 0..10: -o denoised, <name>.noisy.png as rendered>]\n"
          "          [-e <adaptive sampling: tiles whose error estimate is <= this stop early; -s is the budget; one GPU>]\n"
          "          [-q <x,y: print what the ray through the centre of that pixel hits; nothing is rendered>]\n"
          "          [-u <factor >= 2: render at 1/factor of the size, upsample under full-size first-hit buffers; <name>.low.png>]\n"
          "          [-l <aperture,focus: depth of field from a thin lens of that radius, sharp at that distance; one GPU, trace_path,\n"
          "               not with -p, -e or -u; aperture 0 is the pinhole frame>]\n"
          "          [-k <x,y,z: print the 27 SH9 coefficients of a light probe there, -s rays, -d and -r as given; nothing is rendered>]\n"
          "          [-m <nx,ny,nz[,res]: the probe-lit preview in the frame's place: a grid of that many light probes over the scene, -s rays a\n"
          "               probe; res in 2 .. 32: probes weighed by baked visibility maps of res x res texels; one GPU, not with -p, -e, -u, -l or\n"
          "               -i 1>]\n",
          prog);
}

static int parse_args(int argc, char **argv, Args *a)
{
  for (int i = 1; i < argc; i++)
  {
    if (argv[i][0] != '-' || argv[i][1] == '\0' || i + 1 >= argc)
      return -1;
    const char *val = argv[++i];
    switch (argv[i - 1][1])
    {
    case 'w': a->options.width = atoi(val); break;
    case 'h': a->options.height = atoi(val); break;
    case 's': a->options.samples = atoi(val); break;
    case 'o': a->options.result = (char *)val; break;
    case 'd': a->depth = atoi(val); break;
    case 'c': a->config = atoi(val); break;
    case 'g': a->gpus = atoi(val); break;
    case 'r': a->seed = strtoull(val, NULL, 10); break;
    case 'i': a->integrator = atoi(val); break;
    case 'b':
      if ((val[0] != '0' && val[0] != '1') || val[1] != '\0')
        return -1;
      a->bvh = val[0] - '0';
      break;
    case 'a': a->aov = val; break;
    case 'n':
      a->denoise = atoi(val) + 1;
      if (a->denoise < 1 || a->denoise > 11 || val[0] < '0' || val[0] > '9')
        return -1;
      break;
    case 'e':
      a->adaptive = 1;
      a->threshold = strtod(val, NULL);
      if (!(a->threshold >= 0.0) || (val[0] != '.' && (val[0] < '0' || val[0] > '9')))
        return -1;
      break;
    case 'q':
    {
      char *end = NULL;
      a->qx = strtod(val, &end);
      if (end == val || *end != ',')
        return -1;
      const char *second = end + 1;
      a->qy = strtod(second, &end);
      if (end == second || *end != '\0' || !(a->qx >= 0) || !(a->qy >= 0) || a->qx != floor(a->qx) || a->qy != floor(a->qy))
        return -1;
      a->query = 1;
      break;
    }
    case 'l':
    {
      char *end = NULL;
      a->lens_aperture = strtod(val, &end);
      if (end == val || *end != ',')
        return -1;
      const char *second = end + 1;
      a->lens_focus = strtod(second, &end);
      if (end == second || *end != '\0' || !(a->lens_aperture >= 0) || !(a->lens_focus > 0))
        return -1;
      a->lens = 1;
      break;
    }
    case 'k':
    {
      const char *at = val;
      for (int c = 0; c < 3; c++)
      {
        char *end = NULL;
        a->probe_at[c] = strtod(at, &end);
        if (end == at || *end != (c < 2 ? ',' : '\0') || !isfinite(a->probe_at[c]))
          return -1;
        at = end + 1;
      }
      a->probe = 1;
      break;
    }
    case 'm':
    {
      const char *at = val;
      for (int c = 0; c < 3; c++)
      {
        char *end = NULL;
        const long n = strtol(at, &end, 10);
        if (end == at || (c < 2 ? *end != ',' : (*end != ',' && *end != '\0')) || n < 1 || n > (1 << 24))
          return -1;
        a->grid[c] = (int)n;
        at = end + (*end ? 1 : 0);
      }
      a->grid_vis = 0;
      if (*at || at[-1] == ',')
      { /* the optional fourth number: the visibility maps' resolution */
        char *end = NULL;
        const long res = strtol(at, &end, 10);
        if (end == at || *end != '\0' || res < 2 || res > 32)
          return -1;
        a->grid_vis = (int)res;
      }
      break;
    }
    case 'u':
      a->upsample = atoi(val);
      if (a->upsample < 2 || val[0] < '0' || val[0] > '9')
        return -1;
      break;
    case 'p':
      a->pass = atoi(val);
      if (a->pass < 1)
        return -1; /* -p 0 (or not a number) */
      break;
    default: return -1;
    }
  }
  return 0;
}

/* the scene's meshes as the shim takes them; the caller frees */
static RtHipMesh *hip_meshes_of(const RtSceneInfo *info, const MeshObject *meshes)
{
  RtHipMesh *hm = (RtHipMesh *)calloc(info->n_meshes ? info->n_meshes : 1, sizeof *hm);
  for (size_t m = 0; hm && m < info->n_meshes; m++)
  {
    hm[m].flags = meshes[m].flags;
    memcpy(hm[m].color, &meshes[m].color, sizeof hm[m].color);
    memcpy(hm[m].emission, &meshes[m].emission, sizeof hm[m].emission);
    hm[m].num_triangles = meshes[m].mesh.num_triangles;
    hm[m].vertices = (const RtHipVertex *)meshes[m].mesh.vertices;
  }
  return hm;
}

/* -q: one camera ray through the shim's query entry point for C hosts */
static int query_pixel(const Args *a, const RtSceneInfo *info, const Object *scene, const MeshObject *meshes, const Camera *camera)
{
  if (a->qx >= a->options.width || a->qy >= a->options.height)
  {
    fprintf(stderr, "-q %g,%g: outside the %d x %d image\n", a->qx, a->qy, a->options.width, a->options.height);
    return EXIT_FAILURE;
  }
  RtHipMesh *hm = hip_meshes_of(info, meshes);
  if (!hm)
    return EXIT_FAILURE;
  const double uv[2] = {(a->qx + 0.5) / ((double)a->options.width - 1.0), (a->qy + 0.5) / ((double)a->options.height - 1.0)};
  const double *c = &camera->position.x;
  RtHipQueryParams p;
  rt_hip_query_defaults(&p);
  p.source = RT_HIP_RAYS_CAMERA_UV;
  p.camera = (const RtHipCamera *)camera;
  p.origin_radius = sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
  uint32_t status = 0, object = 0, prim = 0;
  double t = 0, point[3], normal[3];
  const RtHipHits h = {&status, &t, &object, &prim, point, normal, NULL, NULL};
  const int rc = rt_hip_query_rays_host((const RtHipSphere *)scene, info->n_objects, hm, info->n_meshes, uv, NULL, 1, &p, 0, &h);
  free(hm);
  if (rc)
  {
    fprintf(stderr, "query: GPU path failed (%d): %s\n", rc, rt_hip_last_error());
    return EXIT_FAILURE;
  }
  printf("pixel = %.0f,%.0f\n", a->qx, a->qy);
  printf("status = %u (%s)\n", status, status == 1 ? "hit" : (status == 0 ? "miss" : "invalid ray"));
  if (status == 1)
  {
    printf("object = %u\n", object);
    if (prim != 0xFFFFFFFFu)
      printf("primitive = %u\n", prim);
    else
      printf("primitive = none (a sphere)\n");
    printf("t = %.17g\n", t);
    printf("point = %.17g %.17g %.17g\n", point[0], point[1], point[2]);
    printf("normal = %.17g %.17g %.17g\n", normal[0], normal[1], normal[2]);
  }
  return EXIT_SUCCESS;
}

/* -k: one light probe through the shim's bake entry point for C hosts */
static int probe_point(const Args *a, const RtSceneInfo *info, const Object *scene, const MeshObject *meshes)
{
  RtHipMesh *hm = hip_meshes_of(info, meshes);
  if (!hm)
    return EXIT_FAILURE;
  const double *c = a->probe_at;
  RtHipProbeParams p;
  rt_hip_probe_defaults(&p);
  p.samples = a->options.samples;
  p.max_depth = a->depth;
  p.seed = a->seed;
  p.origin_radius = sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
  double coeff[27];
  uint32_t status = 0;
  const int rc = rt_hip_bake_probes_host((const RtHipSphere *)scene, info->n_objects, hm, info->n_meshes, c, NULL, 1, &p, 0, coeff, NULL, &status, NULL);
  free(hm);
  if (rc)
  {
    fprintf(stderr, "probe: GPU path failed (%d): %s\n", rc, rt_hip_last_error());
    return EXIT_FAILURE;
  }
  printf("probe = %.17g,%.17g,%.17g\n", c[0], c[1], c[2]);
  printf("samples = %d\n", p.samples);
  printf("status = %u\n", status);
  for (int j = 0; j < 9; j++)
    printf("sh[%d] = %.17g %.17g %.17g\n", j, coeff[3 * j], coeff[3 * j + 1], coeff[3 * j + 2]);
  return EXIT_SUCCESS;
}

/* -u: the frame at 1 / f of the size, its first-hit buffers at both sizes, the guided upsampling */
static int upsample_preview(const Args *a, const RtSceneInfo *info, Object *scene, MeshObject *meshes, Camera *camera)
{
  const int w = a->options.width, h = a->options.height, f = a->upsample;
  const int wl = (w + f - 1) / f, hl = (h + f - 1) / f;
  if (wl < 2 || hl < 2)
  {
    fprintf(stderr, "-u %d: the low frame would be %d x %d; both sides must be at least 2\n", f, wl, hl);
    return EXIT_FAILURE;
  }
  const size_t n = (size_t)w * (size_t)h, nl = (size_t)wl * (size_t)hl;
  char low_path[4096];
  const size_t len = strlen(a->options.result);
  const size_t stem = len >= 4 && strcmp(a->options.result + len - 4, ".png") == 0 ? len - 4 : len;
  /* one block of floats: per frame albedo, normal (3), depth, hits (1); the low colour twice (as rendered, denoised) */
  float *block = (float *)malloc((8 * (n + nl) + 6 * nl) * sizeof(float));
  uint8_t *fb = (uint8_t *)calloc(3 * (n + nl), 1);
  if (!block || !fb || snprintf(low_path, sizeof low_path, "%.*s.low.png", (int)stem, a->options.result) >= (int)sizeof low_path)
  {
    fprintf(stderr, "could not allocate the frames or name the low PNG (-u)\n");
    free(block);
    free(fb);
    return EXIT_FAILURE;
  }
  float *at = block;
  RtAovImage aov[2]; /* low, full */
  const size_t count[2] = {nl, n};
  for (int k = 0; k < 2; k++)
  {
    aov[k].albedo = at;
    aov[k].normal = at + 3 * count[k];
    aov[k].depth = at + 6 * count[k];
    aov[k].hits = (uint32_t *)(at + 7 * count[k]);
    aov[k].object_id = NULL;
    at += 8 * count[k];
  }
  float *linear_low = at, *denoised_low = at + 3 * nl;
  uint8_t *fb_low = fb + 3 * n;
  Options low = a->options, full = a->options;
  low.width = wl;
  low.height = hl;
  int status = EXIT_SUCCESS;
  const double tic = now_seconds();
  render_ex(fb_low, linear_low, scene, info->n_objects, meshes, info->n_meshes, camera, &low);
  const double kernel_s = rt_last_render_seconds();
  const float *colour = linear_low;
  if (rt_last_render_cancelled())
  {
    fprintf(stderr, "not upsampled: the low frame is incomplete\n");
    status = EXIT_FAILURE;
  }
  else if (render_aov(&aov[0], scene, info->n_objects, meshes, info->n_meshes, camera, &low) < 0 ||
           render_aov(&aov[1], scene, info->n_objects, meshes, info->n_meshes, camera, &full) < 0)
    status = EXIT_FAILURE;
  if (status == EXIT_SUCCESS && a->denoise)
  {
    RtHipDenoiseParams dp;
    rt_hip_denoise_defaults(&dp);
    dp.iterations = a->denoise - 1;
    if (denoise_frame(fb_low, denoised_low, linear_low, &aov[0], wl, hl, &dp) != 0)
      status = EXIT_FAILURE;
    colour = denoised_low;
  }
  if (status == EXIT_SUCCESS && upsample_frame(fb, NULL, NULL, colour, &aov[0], wl, hl, &aov[1], w, h, NULL) != 0)
    status = EXIT_FAILURE;
  if (status == EXIT_SUCCESS)
  {
    printf("%d x %d (%d) pixels from %d x %d (-u %d%s)\n", w, h, w * h, wl, hl, f, a->denoise ? ", denoised at the low size" : "");
    printf("cast %lld rays\n", ray_count);
    printf("checked %lld possible intersections\n", intersection_test_count);
    printf("rendering and upsampling took %f seconds (GPU kernels of the low frame %f s)\n", now_seconds() - tic, kernel_s);
    printf("writing result to '%s' and the low frame to '%s'...\n", a->options.result, low_path);
    if (stbi_write_png(a->options.result, w, h, 3, fb, w * 3) == 0 || stbi_write_png(low_path, wl, hl, 3, fb_low, wl * 3) == 0)
      status = EXIT_FAILURE;
    else
      printf("done.\n");
  }
  else
    fprintf(stderr, "could not make the preview (-u %d)\n", f);
  free(block);
  free(fb);
  return status;
}

int main(int argc, char **argv)
{
  Args a;
  memset(&a, 0, sizeof a);
  a.options.width = 320; /* reference main.c:24-30 */
  a.options.height = 180;
  a.options.samples = 50;
  a.options.result = "result.png";
  a.options.obj = "assets/cube.obj";
  a.depth = MAX_DEPTH;
  a.config = 4;
  a.gpus = 1;
  a.seed = 1666943821ull;

  if (argc <= 1 || parse_args(argc, argv, &a) != 0)
  {
    usage(argv[0]);
    return EXIT_FAILURE;
  }
  RtSceneInfo info;
  if (rt_scene_info(a.config, &info) != 0 || a.options.width < 2 || a.options.height < 2 || a.options.samples < 1 ||
      (a.integrator != RT_TRACE_PATH && a.integrator != RT_CAST_RAY) ||
      (a.pass > 0 && (a.pass > a.options.samples || a.gpus > 1)) || (a.adaptive && (a.pass > 0 || a.gpus > 1)) ||
      (a.lens && a.lens_aperture > 0 && (a.pass > 0 || a.adaptive || a.upsample || a.gpus > 1 || a.integrator != RT_TRACE_PATH)) ||
      (a.grid[0] && (a.pass > 0 || a.adaptive || a.upsample || a.gpus > 1 || a.integrator != RT_TRACE_PATH || (a.lens && a.lens_aperture > 0) ||
                     (long long)a.grid[0] * a.grid[1] * a.grid[2] > (1 << 24))))
  {
    usage(argv[0]);
    return EXIT_FAILURE;
  }
  if (a.upsample && (a.gpus > 1 || a.adaptive || a.query || a.pass > 0 || a.aov))
  {
    fprintf(stderr, "-u renders a preview on one GPU: it does not go with -g > 1, -e, -q, -p or -a\n");
    return EXIT_FAILURE;
  }
  printf("seed = %llu\n", (unsigned long long)a.seed);

  Object *scene = (Object *)calloc(info.n_objects ? info.n_objects : 1, sizeof(Object));
  MeshObject *meshes = (MeshObject *)calloc(info.n_meshes ? info.n_meshes : 1, sizeof(MeshObject));
  size_t fb_len = (size_t)a.options.width * (size_t)a.options.height * 3;
  uint8_t *framebuffer = (uint8_t *)calloc(fb_len, 1);
  if (!scene || !meshes || !framebuffer ||
      rt_scene_build(a.config, a.options.width, a.options.height, scene, meshes) != 0)
  {
    fprintf(stderr, "could not allocate framebuffer or scene\n");
    return EXIT_FAILURE;
  }
  signal(SIGINT, on_sigint);
  rt_set_cancel_flag(&interrupted);

  Camera camera;
  vec3 pos = {info.cam_pos[0], info.cam_pos[1], info.cam_pos[2]};
  vec3 target = {info.cam_target[0], info.cam_target[1], info.cam_target[2]};
  init_camera(&camera, pos, target, &a.options);

  if (a.query)
    return query_pixel(&a, &info, scene, meshes, &camera);
  if (a.probe)
    return probe_point(&a, &info, scene, meshes);

  rt_set_max_depth(a.depth);
  rt_set_seed(a.seed);
  rt_set_devices(a.gpus);
  rt_set_integrator(a.integrator);
  rt_set_bvh_builder(a.bvh);
  if (a.lens)
    rt_set_lens(a.lens_aperture, a.lens_focus);
  if (a.grid[0])
    rt_set_probe_grid(a.grid[0], a.grid[1], a.grid[2]);
  rt_set_probe_visibility(a.grid[0] ? a.grid_vis : 0);

  if (a.upsample)
  {
    const int rc = upsample_preview(&a, &info, scene, meshes, &camera);
    rt_scene_free_meshes(meshes, info.n_meshes);
    free(meshes);
    free(scene);
    free(framebuffer);
    return rc;
  }

  /* the process's phase clock (bench.py's cli_host entry reads the `phases:` line): the HIP runtime comes up at the first
   * device query; render_ex's own split is the shim's (rt_hip_last_image_phases) */
  const double t_start = now_seconds();
  (void)rt_hip_device_count();
  const double t_hip = now_seconds();

  /* -n: the frame's linear mean is the denoiser's input; the PNG of the frame as rendered goes to <name>.noisy.png */
  const size_t n_px = (size_t)a.options.width * (size_t)a.options.height;
  float *linear = a.denoise ? (float *)malloc(n_px * 3 * sizeof(float)) : NULL;
  char noisy_path[4096];
  const char *frame_path = a.options.result;
  if (a.denoise)
  {
    const size_t len = strlen(a.options.result);
    const size_t stem = len >= 4 && strcmp(a.options.result + len - 4, ".png") == 0 ? len - 4 : len;
    if (!linear || snprintf(noisy_path, sizeof noisy_path, "%.*s.noisy.png", (int)stem, a.options.result) >= (int)sizeof noisy_path)
    {
      fprintf(stderr, "could not allocate the linear frame or name the noisy PNG (-n)\n");
      return EXIT_FAILURE;
    }
    frame_path = noisy_path;
  }

  double tic = now_seconds();
  int held = a.options.samples;
  if (a.adaptive)
  {
    const size_t n_tiles = (size_t)((a.options.width + 7) / 8) * (size_t)((a.options.height + 7) / 8);
    uint32_t *counts = (uint32_t *)calloc(n_tiles, sizeof(uint32_t));
    RtHipAdaptParams ap;
    rt_hip_adapt_defaults(&ap);
    ap.threshold = a.threshold;
    held = counts ? render_adaptive(framebuffer, linear, counts, scene, info.n_objects, meshes, info.n_meshes, &camera, &a.options, &ap,
                                    on_checkpoint, NULL)
                  : -1;
    if (held < 0)
      return EXIT_FAILURE; /* render_adaptive said why */
    size_t full = 0;
    for (size_t k = 0; k < n_tiles; k++)
      full += counts[k] >= (uint32_t)a.options.samples;
    printf("adaptive: threshold %g, mean %.2f samples per pixel of %d, %.1f %% of the tiles ran the whole budget\n", a.threshold,
           (double)rt_last_pixel_samples() / ((double)a.options.width * a.options.height), a.options.samples,
           100.0 * (double)full / (double)n_tiles);
    free(counts);
  }
  else if (a.pass > 0)
  {
    held = render_progressive(framebuffer, linear, scene, info.n_objects, meshes, info.n_meshes, &camera, &a.options, a.pass,
                              on_pass, NULL);
    if (held < 0)
      return EXIT_FAILURE; /* render_progressive said why */
  }
  else
    render_ex(framebuffer, linear, scene, info.n_objects, meshes, info.n_meshes, &camera, &a.options);
  double toc = now_seconds();
  double phase[3] = {0, 0, 0};
  rt_hip_last_image_phases(phase);

  const double kernel_s = rt_last_render_seconds();
  printf("%d x %d (%d) pixels\n", a.options.width, a.options.height, a.options.width * a.options.height);
  printf("cast %lld rays\n", ray_count);
  printf("checked %lld possible intersections\n", intersection_test_count);
  printf("rendering took %f seconds (GPU kernels %f s on %d GPU%s)\n", toc - tic, kernel_s, a.gpus,
         a.gpus == 1 ? "" : "s");
  if (kernel_s > 0)
    printf("%.3e ray-bounces/s, %.2f Mpixel-samples/s\n", (double)rt_last_ray_bounces() / kernel_s,
           (a.adaptive ? (double)rt_last_pixel_samples() : (double)a.options.width * a.options.height * held) / kernel_s * 1e-6);
  int status = EXIT_SUCCESS;
  if (rt_last_render_cancelled() && (a.pass > 0 || a.adaptive))
    printf("interrupted: the image holds %d of %d samples per pixel\n", held, a.options.samples);
  else if (rt_last_render_cancelled())
    printf("interrupted: the image holds the tiles finished so far\n");
  printf("writing result to '%s'...\n", frame_path);
#ifndef VALGRIND
  if (stbi_write_png(frame_path, a.options.width, a.options.height, 3, framebuffer, a.options.width * 3) == 0)
    status = EXIT_FAILURE;
  else
    printf("done.\n");
#endif
  /* the first-hit buffers of -a and -n hold the frame's own samples: as many as the image holds -- of an adaptive frame the
   * BUDGET's (its tiles hold prefixes of them), unless it was interrupted: then the samples done */
  const int aov_samples = a.adaptive && !rt_last_render_cancelled() ? a.options.samples : held;
  if (a.aov && status == EXIT_SUCCESS)
  { /* the frame's own samples: as many as the image holds, the same seed */
    float *albedo = (float *)malloc(n_px * 3 * sizeof(float)), *normal = (float *)malloc(n_px * 3 * sizeof(float));
    float *depth = (float *)malloc(n_px * sizeof(float));
    RtAovImage aov = {albedo, normal, depth, NULL, NULL};
    Options o = a.options;
    o.samples = aov_samples;
    if (!albedo || !normal || !depth || render_aov(&aov, scene, info.n_objects, meshes, info.n_meshes, &camera, &o) < 0 ||
        write_pfm(a.aov, "albedo", albedo, o.width, o.height, 3) || write_pfm(a.aov, "normal", normal, o.width, o.height, 3) ||
        write_pfm(a.aov, "depth", depth, o.width, o.height, 1))
    {
      fprintf(stderr, "could not write the feature buffers (-a %s)\n", a.aov);
      status = EXIT_FAILURE;
    }
    free(albedo);
    free(normal);
    free(depth);
  }
  if (a.denoise && status == EXIT_SUCCESS)
  {
    if (held < 1 || (rt_last_render_cancelled() && a.pass == 0 && !a.adaptive))
    { /* a one-shot frame cut short holds finished tiles only: nothing to denoise */
      fprintf(stderr, "not denoised: the frame is incomplete\n");
      status = EXIT_FAILURE;
    }
    else
    {
      float *albedo = (float *)malloc(n_px * 3 * sizeof(float)), *normal = (float *)malloc(n_px * 3 * sizeof(float));
      float *depth = (float *)malloc(n_px * sizeof(float));
      uint32_t *hits = (uint32_t *)malloc(n_px * sizeof(uint32_t));
      RtAovImage aov = {albedo, normal, depth, NULL, hits};
      Options o = a.options;
      o.samples = aov_samples;
      RtHipDenoiseParams dp;
      rt_hip_denoise_defaults(&dp);
      dp.iterations = a.denoise - 1;
      const double t0 = now_seconds();
      if (!albedo || !normal || !depth || !hits || render_aov(&aov, scene, info.n_objects, meshes, info.n_meshes, &camera, &o) < 0 ||
          denoise_frame(framebuffer, NULL, linear, &aov, o.width, o.height, &dp) != 0)
      {
        fprintf(stderr, "could not denoise the frame (-n %d)\n", a.denoise - 1);
        status = EXIT_FAILURE;
      }
      else
      {
        printf("denoised (%d iterations, first-hit buffers of %d samples) in %f s; writing '%s'...\n", dp.iterations, aov_samples,
               now_seconds() - t0, a.options.result);
        if (stbi_write_png(a.options.result, o.width, o.height, 3, framebuffer, o.width * 3) == 0)
          status = EXIT_FAILURE;
      }
      free(albedo);
      free(normal);
      free(depth);
      free(hits);
    }
  }
  printf("phases: HIP runtime start %.6f s, context %.6f s, render %.6f s, copy out %.6f s, PNG %.6f s\n", t_hip - t_start, phase[0],
         phase[1], phase[2], now_seconds() - toc);
  rt_scene_free_meshes(meshes, info.n_meshes);
  free(meshes);
  free(scene);
  free(framebuffer);
  free(linear);
  return status;
}

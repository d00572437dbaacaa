/* rt_hip_shim.hip -- the C-ABI of include/rt_hip.h over the kernels of
 * pt_kernel.hip and its sibling units.  Thin by design: argument checks, the one-time conversion of
 * the reference's scene structs (Object raytracer.h:104-111, Vertex :61) into
 * the kernel's HBM layout (pt_device.h), launches, and the single-process
 * multi-GPU gather.  No CPU rendering path exists here: every failure is
 * reported, never papered over.
 */
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <mutex>
#include <new>
#include <utility>
#include <vector>

#include "pt_device.h"
#include "rt_hip.h"
#include "rt_rng.h"
#include "bvh_build.h"
#include "rt_staging.h"

static_assert(sizeof(RtHipSphere) == 88, "RtHipSphere must match the reference Object");
static_assert(sizeof(RtHipVertex) == 40, "RtHipVertex must match the reference Vertex");
static_assert(sizeof(RtHipCamera) == 96, "RtHipCamera must match the reference Camera");
static_assert(RT_HIP_TILE == PT_TILE && RT_HIP_TILE_PIXELS == PT_TILE_PIXELS, "tile shape");
/* exact_triangle<UNSCALED> divides through rcp_unscaled, valid for 2^-500 <= |a| <= 2^500 with |a| <= |e1||e2||d|: a launch
 * refuses near_R >= RT_NEAR_R_LIMIT, vertices lie within near_R / 1.5, so |e1|, |e2| < 2 near_R / 1.5 and |d| <= 1.0001 */
#define RT_NEAR_R_LIMIT 1e15
static_assert((2.0 * RT_NEAR_R_LIMIT / 1.5) * (2.0 * RT_NEAR_R_LIMIT / 1.5) * 1.0001 < 3.2e150 /* < 2^500 */,
              "the near_R limit keeps |e1||e2||d| inside rcp_unscaled's range");

namespace
{

thread_local char g_err[512] = "";
const volatile int *g_cancel = nullptr; /* rt_hip_set_cancel_flag */

int fail(int code, const char *fmt, ...)
{
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
  return code;
}

/* what a kernel launch gave as the call's answer: RT_HIP_OK, or RT_HIP_ERUNTIME naming the kernel */
int launched(hipError_t e, const char *kernel)
{
  return e == hipSuccess ? (int)RT_HIP_OK : fail(RT_HIP_ERUNTIME, "%s launch: %s", kernel, hipGetErrorString(e));
}

#define HIP_TRY(expr)                                                                               \
  do                                                                                                \
  {                                                                                                 \
    hipError_t e_ = (expr);                                                                         \
    if (e_ != hipSuccess)                                                                           \
    {                                                                                               \
      (void)hipGetLastError(); /* reported here: no later call may find it again */                 \
      return fail(e_ == hipErrorOutOfMemory ? RT_HIP_ENOMEM : RT_HIP_ERUNTIME, "%s: %s", #expr,     \
                  hipGetErrorString(e_));                                                           \
    }                                                                                               \
  } while (0)

#define NCCL_TRY(expr)                                                                              \
  do                                                                                                \
  {                                                                                                 \
    ncclResult_t r_ = (expr);                                                                       \
    if (r_ != ncclSuccess)                                                                          \
      return fail(RT_HIP_ERUNTIME, "%s: %s", #expr, ncclGetErrorString(r_));                        \
  } while (0)

/* selects a device for the current scope and puts the previous one back */
struct DeviceScope
{
  int prev = -1;
  hipError_t status;
  explicit DeviceScope(int device)
  {
    status = hipGetDevice(&prev);
    if (status == hipSuccess && prev != device)
      status = hipSetDevice(device);
  }
  ~DeviceScope()
  {
    if (prev >= 0)
      (void)hipSetDevice(prev);
  }
};

/* A device allocation that is freed when its owner -- a scope, or a longer-lived object that has it as a member -- goes away.
 * alloc() reports as hipMalloc does and leaves no sticky error behind a failure (the caller may go on with less: a later
 * hipGetLastError() must not see it).  at<T>(byte offset) is the typed view of a part.  Movable, not copyable. */
struct DeviceBuffer
{
  void *ptr = nullptr;
  DeviceBuffer() = default;
  DeviceBuffer(DeviceBuffer &&o) noexcept { std::swap(ptr, o.ptr); }
  DeviceBuffer &operator=(DeviceBuffer &&o) noexcept
  {
    std::swap(ptr, o.ptr); /* what this one held goes with `o` */
    return *this;
  }
  ~DeviceBuffer() { release(); }
  hipError_t alloc(size_t bytes)
  {
    release();
    const hipError_t e = hipMalloc(&ptr, bytes);
    if (e != hipSuccess)
    {
      ptr = nullptr;
      (void)hipGetLastError();
    }
    return e;
  }
  void release()
  {
    if (ptr)
      (void)hipFree(ptr);
    ptr = nullptr;
  }
  explicit operator bool() const { return ptr != nullptr; }
  template <class T>
  T *at(size_t byte_offset = 0) const
  {
    return reinterpret_cast<T *>(static_cast<char *>(ptr) + byte_offset);
  }
};

/* The one device allocation of a host-array entry point, laid out by StagePlan (rt_staging.h).  A host form declares its parts,
 * stage()s them -- the allocation, the cleared parts, the uploads, in declared order --, launches on the null stream with at<T>()'s
 * pointers (null for a part the call does not want) and download()s: the null stream puts those copies after the kernel. */
struct StageArena
{
  StagePlan plan;
  DeviceBuffer buf;
  int part(size_t bytes, const void *src = nullptr, void *dst = nullptr, bool wanted = true) { return plan.add(bytes, src, dst, wanted); }
  int zeroed(size_t bytes, void *dst) { return plan.add(bytes, nullptr, dst, true, true); }
  template <class T>
  T *at(int part) const
  {
    const size_t off = plan.offset(part);
    return off == STAGE_ABSENT ? nullptr : buf.at<T>(off);
  }
  int stage()
  {
    HIP_TRY(buf.alloc(plan.total));
    for (const StagePart &p : plan.parts)
    {
      if (p.zero)
        HIP_TRY(hipMemset(buf.at<char>(p.offset), 0, p.bytes));
      if (p.src)
        HIP_TRY(hipMemcpy(buf.at<char>(p.offset), p.src, p.bytes, hipMemcpyHostToDevice));
    }
    return RT_HIP_OK;
  }
  int download() const
  {
    for (const StagePart &p : plan.parts)
      if (p.dst)
        HIP_TRY(hipMemcpy(p.dst, buf.at<char>(p.offset), p.bytes, hipMemcpyDeviceToHost));
    return RT_HIP_OK;
  }
};

/* The parts of a radiance query's or a pixel refinement's host form behind its input: the requested outputs, then the counters,
 * cleared.  The device's RtHipRadiance once the arena is staged, and the counters added to the caller's after the download. */
struct RadianceStage
{
  int out[6], stats;
  uint64_t st[RT_HIP_NSTATS];
  uint64_t *h_stats;
  RadianceStage(const RadianceStage &) = delete; /* (the plan points into st) */
  RadianceStage(StageArena &A, const RtHipRadiance *h, uint64_t n, int32_t samples, uint64_t *h_stats_) : h_stats(h_stats_)
  {
    void *host[6] = {h->status, h->radiance, h->samples, h->paths, h->casts, h->ray};
    const size_t bytes_per_entry[6] = {4, 24, 24u * (size_t)samples, 8, 8, 48};
    for (int k = 0; k < 6; k++)
      out[k] = A.part(bytes_per_entry[k] * n, nullptr, host[k], host[k] != nullptr);
    stats = A.zeroed(sizeof st, h_stats ? st : nullptr);
  }
  RtHipRadiance device(const StageArena &A) const
  {
    return {A.at<uint32_t>(out[0]), A.at<double>(out[1]), A.at<double>(out[2]), A.at<uint64_t>(out[3]), A.at<uint64_t>(out[4]), A.at<double>(out[5])};
  }
  int download(const StageArena &A) const
  {
    const int rc = A.download();
    for (int k = 0; !rc && h_stats && k < RT_HIP_NSTATS; k++)
      h_stats[k] += st[k];
    return rc;
  }
};

/* The first-hit buffers an image-space host form reads: the channels of an n-pixel RtHipAov as uploaded parts, declared in the
 * order albedo, normal, depth, hits, object -- albedo and object where the call's flags want them, nothing at all without `have`
 * (a history that is not given).  The device's RtHipAov once the arena is staged: null for a channel that has no part. */
struct AovStage
{
  int albedo, normal, depth, hits, object; /* (initialised in this order) */
  AovStage(StageArena &A, const RtHipAov *h, size_t n, bool want_albedo, bool want_object, bool have = true)
      : albedo(A.part(12u * n, h->albedo, nullptr, have && want_albedo)), normal(A.part(12u * n, h->normal, nullptr, have)),
        depth(A.part(4u * n, h->depth, nullptr, have)), hits(A.part(4u * n, h->hits, nullptr, have)),
        object(A.part(4u * n, h->object, nullptr, have && want_object))
  {
  }
  RtHipAov device(const StageArena &A) const
  {
    return {A.at<float>(albedo), A.at<float>(normal), A.at<float>(depth), A.at<uint32_t>(object), A.at<uint32_t>(hits)};
  }
};

/* a scene of a host form's own on a HIP device: destroyed when the scope ends */
struct OwnedScene
{
  RtHipScene *scene = nullptr;
  OwnedScene() = default;
  OwnedScene(const OwnedScene &) = delete;
  OwnedScene &operator=(const OwnedScene &) = delete;
  ~OwnedScene() { rt_hip_scene_destroy(scene); }
  int create(const RtHipSphere *spheres, size_t n_spheres, const RtHipMesh *meshes, size_t n_meshes, int device)
  {
    return rt_hip_scene_create(spheres, n_spheres, meshes, n_meshes, device, &scene);
  }
};

/* Two timing events around a piece of work on one stream.  Movable, not copyable. */
struct EventPair
{
  hipEvent_t ev[2] = {nullptr, nullptr};
  EventPair() = default;
  EventPair(EventPair &&o) noexcept { std::swap(ev, o.ev); }
  EventPair &operator=(EventPair &&o) noexcept
  {
    std::swap(ev, o.ev);
    return *this;
  }
  ~EventPair()
  {
    for (hipEvent_t x : ev)
      if (x)
        (void)hipEventDestroy(x);
  }
  hipError_t create()
  {
    const hipError_t e = hipEventCreate(&ev[0]);
    return e == hipSuccess ? hipEventCreate(&ev[1]) : e;
  }
  hipError_t start(hipStream_t stream) { return hipEventRecord(ev[0], stream); }
  hipError_t stop(hipStream_t stream) { return hipEventRecord(ev[1], stream); }
  hipError_t wait() { return hipEventSynchronize(ev[1]); } /* for the stop */
  hipError_t elapsed_ms(float *ms) { return hipEventElapsedTime(ms, ev[0], ev[1]); }
};

/* C++ exceptions (std::bad_alloc from a std::vector, above all) must not cross the C boundary: every entry point whose body can
 * throw runs it in here */
template <class F>
int guarded(const char *name, F &&body)
{
  try
  {
    return body();
  }
  catch (const std::bad_alloc &)
  {
    return fail(RT_HIP_ENOMEM, "host allocation failed in %s", name);
  }
  catch (...)
  {
    return fail(RT_HIP_ERUNTIME, "unexpected C++ exception in %s", name);
  }
}

} // namespace

/* The camera-dependent tables of a scene (packed-fp32 filter table, fp32 hierarchy nodes; both
 * depend on near_R, i.e. on the camera's distance) for one near_R.  Built once on the stream of
 * the first launch that needs them and immutable afterwards, so launches of one scene with
 * different cameras on different streams or threads never write a table another launch reads;
 * later launches on other streams wait on `built`.  A scene keeps up to RT_TABLE_SETS of them;
 * beyond that the least recently used one is recycled after every stream that read it (`readers`) is done. */
struct TableSet
{
  double near_R = 0;
  float *filt = nullptr, *bvh_nodes = nullptr;
  hipEvent_t built = nullptr;
  /* one "last read" event PER READER STREAM: a single event re-recorded by whichever launch releases last would
   * forget the readers on other streams (an event holds only its latest record), and the set could be recycled
   * under a kernel that still reads it (round-2 advisor finding) */
  std::vector<std::pair<hipStream_t, hipEvent_t>> readers;
  uint64_t stamp = 0;
  int users = 0;      /* launches between acquire_tables() and release_tables(): not recyclable */
  bool owned = false; /* allocated apart from the scene blob */
};
#define RT_TABLE_SETS 8

struct RtHipScene
{
  int device = 0;
  PtSceneView view{}; /* view.filt / view.bvh_nodes: storage of table set 0, inside the blob */
  mutable std::mutex table_mutex;
  mutable std::vector<TableSet> tables;
  mutable uint64_t table_clock = 0;
  size_t filt_bytes = 0, bvh_nodes_bytes = 0;
  /* workspace of the parked-walk kernels (scenes with a triangle hierarchy): in-use flags, then the rings
   * (pt_device.h).  ONE per device, shared by every scene on it and counted (park_acquire_ws / park_drop_ws): the 385 MB (round 4: 462; round 3: 406)
   * used to be allocated per scene -- a test suite's every 48 x 32 fuzz scene paid it, and scenes alive at the same
   * time each held a copy (round-3 advisor finding).  Sharing is safe between concurrent launches of different scenes:
   * a workgroup takes a slot with an atomic flag, and the pool has more slots per XCD than workgroups can be resident. */
  mutable char *park_ws = nullptr;
  mutable uint32_t park_slots_per_xcd = 0;
  mutable bool park_tried = false;
  void *blob = nullptr; /* one device allocation holding every array */
  double reach = 0;     /* >= |p| for every point p on a primitive of ordinary size (radius < 1000) */
  double max_emission = 0; /* max |emission component| over all materials */
  bool any_mirror_glass = false; /* a material with M_REFLECTION and M_REFRACTION: cast_ray traces two children */
  double max_center = 0; /* max |centre| over the spheres (rounded up) */
  /* the scene's LEADING wall-sized spheres (radius >= 1000), whole pairs of them, at most 2 PT_BIG_PAIRS: radius and
   * |centre| -- what big_prune_for needs to bound their hit-distance estimates (pt_filter.h, BigPrune) */
  int n_big = 0;
  double big_r[8] = {0}, big_c[8] = {0};
  /* bounding sphere of every triangle (bvh_probe): centre, radius, |centre| -- radius < 0: no triangles */
  double mesh_c[3] = {0, 0, 0}, mesh_R = -1, mesh_c_norm = 0;
  bool hull_flags = false; /* tri_object carries PT_HULL_PLUS / PT_HULL_MINUS (pt_build_hull_flags ran) */
  /* the hierarchy's origin (rt_hip_scene_bvh_info): RT_HIP_BVH_*, the least depth its leaves allow, the build's seconds */
  uint32_t bvh_builder = RT_HIP_BVH_HOST, bvh_max_depth = 0;
  double bvh_build_seconds = 0;
  /* ---- moving the triangles in place (rt_hip_scene_update_vertices) ---- */
  size_t blob_bytes = 0;     /* new positions must not lie inside the blob */
  double reach_spheres = 0;  /* the spheres' part of `reach`: joined with the vertices' again by every update */
  double reach_triangles = 0; /* the vertices' part (max |vertex|; 0 without triangles): joined with the spheres' by rt_hip_scene_update_spheres */
  bool force_wide = false;   /* PT_DEV_KERNELS, RT_HIP_FORCE_BIG=1: an OR on top of the wide_range the spheres give */
  mutable std::atomic<int> live_accums{0}; /* RtHipAccum objects on this scene: their plans hold the view, so no update */
  bool unusable = false;     /* an update failed after it had begun to write: only rt_hip_scene_destroy is allowed */
  /* the hierarchy's levels (BvhRefit::levels), made by the first update and kept: they depend on the topology alone */
  uint32_t *refit_by_level = nullptr; /* device memory, n_bvh_nodes */
  std::vector<uint32_t> refit_level_begin;
  uint64_t updates = 0;
  double last_update_seconds = 0;
  /* ---- the topology rebuilt in place (rt_hip_scene_rebuild_bvh) ---- */
  uint32_t bvh_node_capacity = 0; /* nodes that view.bvh_src and view.bvh_nodes have room for */
  void *bvh_side = nullptr;       /* a tree of more nodes than the blob's regions hold: source nodes, then table set 0's fp32 nodes */
  size_t bvh_side_bytes = 0;
  uint64_t rebuilds = 0;
  double last_rebuild_seconds = 0;
  /* the device cost of the tree as it was last built (scene_built_cost; guarded by table_mutex) */
  mutable double built_cost = 0;
  mutable bool built_cost_known = false;
  /* the cost kernel's workspace (scene_tree_cost), kept so that a per-frame question allocates nothing: made at the first cost,
   * replaced when a tree of more nodes is priced; guarded by table_mutex */
  mutable double *cost_ws = nullptr;
  mutable uint32_t cost_ws_nodes = 0;
};

/* ---- progressive rendering: one frame accumulated over passes (rt_hip.h, RtHipAccum) ----------------------------------------
 * The plan is made once, for the whole budget, and every pass launches its member in accumulation mode (PtLaunch.sample_first,
 * acc_keep): the CHUNKS members add exact integer sums (fixed point, or windowed words) to the tile records in `sums`, the static
 * body continues its lanes' fp64 slice sums there.  A pass never re-plans, and the pools the plan needs are held here. */
struct RtHipAccum
{
  const RtHipScene *scene = nullptr;
  PtLaunch L;                  /* the launch as planned at create; a pass sets samples, sample_first, sample_chunks, stats */
  int kernel = -1;
  bool takes_chunks = false;   /* CHUNKS member: sums are tile records (pt_resolve_tiles); else slice sums (pt_resolve_slices) */
  int32_t budget = 0, done = 0;
  int32_t plan_spc = 0;        /* the plan's samples per chunk: no workgroup of a pass gets more */
  /* the sums, the accumulation's own pending-ray pool (pend_pool_own; empty where the plan needs none), and for adaptive sampling
   * the freeze state, allocated at the first freeze (accum_adapt_state) in one block -- per slot the count it froze at (0: live),
   * the live slots in ascending order, their number, the keep mask of a freeze -- and rt_hip_accum_run_adaptive's two compact
   * resolves and the error per slot.  accum_free waits for the device before they go. */
  DeviceBuffer sums, pend, tile_samples, adapt_buf;
  uint32_t *slot_list = nullptr, *d_live_count = nullptr; /* inside tile_samples */
  uint8_t *keep = nullptr;
  uint32_t live_count = 0;     /* host copy; meaningful once tile_samples exists */
  bool any_frozen = false;
  bool broken = false;         /* a freeze failed after the device had rewritten the list: the host's count is stale, nothing may launch */
};

namespace
{

int usable_devices()
{
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess)
  {
    (void)hipGetLastError();
    return 0;
  }
  return n;
}

bool have_device(int device) { return device >= 0 && device < usable_devices(); }

/* One object's `material` record, its color_raw triple, the acceptance rule and every scalar a scene derives from its materials:
 * scene_material_* (bvh_build.h), one text with the device's (rt_hip_scene_update_materials). */

/* One sphere's record of entry_src (pt_device.h), its geom4 copy and every scalar a scene derives from its spheres:
 * scene_sphere_* (bvh_build.h), one text with the device's (rt_hip_scene_update_spheres). */

/* One triangle's records: scene_triangle_entry / scene_triangle_normal (bvh_build.h), one text with the device's. */

/* ---- bounding-volume hierarchy over triangles: BvhBuild, in bvh_build.h (host C++, shared with the CPU test of its invariants) ---- */

/* Fault injection for tests (rt_hip_selftest_fail_alloc): which of the shim's optional device allocations behave as if
 * hipMalloc had failed, so that the fallback kernels are reachable -- and testable -- on a 288 GB device. */
std::atomic<uint32_t> g_fail_alloc{0};

/* the kernel the calling thread's last rt_hip_render_tiles* launched (rt_hip_last_launch_kernel) */
thread_local int g_last_kernel = -1;

size_t pad256(size_t b) { return (b + 255) & ~(size_t)255; }

/* every launch that reads the set is done: its build, and the last read of every stream that ever read it */
hipError_t table_set_wait(const TableSet &t)
{
  hipError_t first = t.built ? hipEventSynchronize(t.built) : hipSuccess;
  for (auto &r : t.readers) /* all of them, whatever one of them says */
    if (const hipError_t e = hipEventSynchronize(r.second); first == hipSuccess)
      first = e;
  return first;
}

/* the set's events and, where it owns them, its tables; the caller has waited */
void table_set_free(TableSet &t)
{
  for (auto &r : t.readers)
    (void)hipEventDestroy(r.second);
  if (t.built)
    (void)hipEventDestroy(t.built);
  if (t.owned)
  {
    (void)hipFree(t.filt);
    (void)hipFree(t.bvh_nodes);
  }
}

/* the one refusal of no scene, and of a scene that a mutation left half written */
int scene_usable(const RtHipScene *scene, const char *who)
{
  if (!scene)
    return fail(RT_HIP_EINVAL, "%s: scene is NULL (a scene is required)", who);
  if (scene->unusable)
    return fail(RT_HIP_ERUNTIME, "the scene is unusable: an update of its vertices, spheres or materials failed half way (rt_hip_scene_update_*)");
  return RT_HIP_OK;
}

/* A scene about to be written -- its vertices, its spheres or its hierarchy -- after scene_usable() and the mutation's own
 * refusals.  The constructor makes the scene's device current (scope.status says how that went); then, in this order:
 *   lock.lock()      table_mutex, held until the scope ends
 *   idle()           refuses while accumulations are alive or a launch is being submitted; `change` is what they must not see
 *   drain()          no launch may still read what is about to change: every table set's build and readers
 *   stale()          writing begins: filter, fp32 nodes and tri32 records are rebuilt by the next launch (acquire_tables)
 *   broke(e, what)   the one exit of a HIP failure after that: only rt_hip_scene_destroy is allowed from here on */
struct SceneWrite
{
  RtHipScene *scene;
  const char *change;
  DeviceScope scope;
  std::unique_lock<std::mutex> lock;
  SceneWrite(RtHipScene *s, const char *change_) : scene(s), change(change_), scope(s->device), lock(s->table_mutex, std::defer_lock) {}
  int idle() const
  {
    if (scene->live_accums.load() > 0)
      return fail(RT_HIP_EINVAL, "%d accumulation(s) on this scene are alive: destroy them before %s", scene->live_accums.load(), change);
    for (const TableSet &t : scene->tables)
      if (t.users > 0)
        return fail(RT_HIP_EINVAL, "a launch of this scene is being submitted");
    return RT_HIP_OK;
  }
  int drain() const
  {
    for (const TableSet &t : scene->tables)
      HIP_TRY(table_set_wait(t));
    return RT_HIP_OK;
  }
  void stale() const
  {
    for (TableSet &t : scene->tables)
      t.near_R = -1.0;
  }
  int broke(hipError_t e, const char *what) const
  {
    (void)hipGetLastError();
    scene->unusable = true;
    return fail(RT_HIP_ERUNTIME, "%s: %s; the scene is unusable now (destroy it)", what, hipGetErrorString(e));
  }
};

/* The table set of `scene` for `near_R`, ready to be read by work submitted to `stream` after this
 * call (see TableSet).  *slot identifies it for release_tables(). */
int acquire_tables(const RtHipScene *scene, double near_R, hipStream_t stream, float **filt, float **bvh_nodes, size_t *slot)
{
  std::lock_guard<std::mutex> lock(scene->table_mutex);
  std::vector<TableSet> &tables = scene->tables;
  if (const int rc = scene_usable(scene, "a launch"))
    return rc;
  for (size_t k = 0; k < tables.size(); k++)
    if (tables[k].near_R == near_R)
    {
      HIP_TRY(hipStreamWaitEvent(stream, tables[k].built, 0));
      tables[k].stamp = ++scene->table_clock;
      tables[k].users++;
      *filt = tables[k].filt;
      *bvh_nodes = tables[k].bvh_nodes;
      *slot = k;
      return RT_HIP_OK;
    }
  size_t k = tables.size();
  for (size_t j = 0; j < tables.size() && k == tables.size(); j++)
    if (tables[j].near_R == -1.0 && tables[j].users == 0)
      k = j; /* a set whose build failed, or that an update of the vertices left stale: rebuilt in place */
  if (k < tables.size())
    HIP_TRY(table_set_wait(tables[k]));
  else if (k < RT_TABLE_SETS)
  {
    TableSet t;
    if (k == 0)
    { /* the storage inside the scene blob */
      t.filt = scene->view.filt;
      t.bvh_nodes = scene->view.bvh_nodes;
    }
    else
    {
      t.owned = true;
      HIP_TRY(hipMalloc(&t.filt, scene->filt_bytes ? scene->filt_bytes : 256));
      hipError_t e = hipMalloc(&t.bvh_nodes, scene->bvh_nodes_bytes ? scene->bvh_nodes_bytes : 256);
      if (e != hipSuccess)
      {
        (void)hipFree(t.filt);
        return fail(RT_HIP_ENOMEM, "hipMalloc of a hierarchy table: %s", hipGetErrorString(e));
      }
    }
    hipError_t e = hipEventCreateWithFlags(&t.built, hipEventDisableTiming);
    if (e != hipSuccess)
    {
      table_set_free(t);
      return fail(RT_HIP_ERUNTIME, "hipEventCreate: %s", hipGetErrorString(e));
    }
    tables.push_back(t);
  }
  else
  {
    /* recycle the least recently used set once every launch that reads it has finished */
    k = tables.size();
    for (size_t j = 0; j < tables.size(); j++)
      if (tables[j].users == 0 && (k == tables.size() || tables[j].stamp < tables[k].stamp))
        k = j;
    if (k == tables.size())
      return fail(RT_HIP_ELIMIT, "more than %d launches of one scene with different camera distances are being submitted at once",
                  RT_TABLE_SETS);
    HIP_TRY(table_set_wait(tables[k]));
  }
  TableSet &t = tables[k];
  t.near_R = near_R;
  t.stamp = ++scene->table_clock;
  {
    hipError_t e = pt_launch_build_tables(scene->view, near_R, t.filt, t.bvh_nodes, stream);
    if (e == hipSuccess) e = hipEventRecord(t.built, stream);
    if (e != hipSuccess)
    {
      t.near_R = -1.0; /* never matches a launch: the set is rebuilt (or recycled) by the next one */
      return fail(RT_HIP_ERUNTIME, "building the filter / hierarchy tables: %s", hipGetErrorString(e));
    }
  }
  t.users++;
  *filt = t.filt;
  *bvh_nodes = t.bvh_nodes;
  *slot = k;
  return RT_HIP_OK;
}

/* after the render that reads table set `slot` has been submitted to `stream` */
void release_tables(const RtHipScene *scene, size_t slot, hipStream_t stream)
{
  std::unique_lock<std::mutex> lock(scene->table_mutex);
  if (slot >= scene->tables.size())
    return;
  hipEvent_t ev = nullptr;
  {
    TableSet &t = scene->tables[slot];
    for (auto &r : t.readers)
      if (r.first == stream)
        ev = r.second;
    if (!ev && t.readers.size() >= 32)
    { /* a caller cycling through many streams: take the oldest reader's event out of the set, wait it out WITHOUT
       * the lock (other threads' launches of this scene go on meanwhile; the set cannot be recycled under the
       * waited-for reader because this launch still counts in `users`), and hand the event to this stream */
      hipEvent_t old = t.readers.front().second;
      t.readers.erase(t.readers.begin());
      lock.unlock();
      (void)hipEventSynchronize(old);
      lock.lock();
      ev = old;
      scene->tables[slot].readers.emplace_back(stream, ev);
    }
    else if (!ev)
    {
      if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) == hipSuccess)
        t.readers.emplace_back(stream, ev);
      else
      { /* no event to remember this reader by: let it finish before the set can be recycled */
        ev = nullptr;
        (void)hipGetLastError();
        lock.unlock();
        (void)hipStreamSynchronize(stream);
        lock.lock();
      }
    }
  }
  TableSet &t = scene->tables[slot]; /* (the vector may have grown while the lock was away) */
  if (ev)
    (void)hipEventRecord(ev, stream);
  t.users--;
}

/* the per-device workspace of the parked-walk kernels (RtHipScene::park_ws) */
struct ParkPool
{
  char *ws = nullptr;
  int users = 0;
  uint32_t slots_per_xcd = 0;
};
std::mutex g_park_mutex;
ParkPool g_park[64];

size_t park_flag_bytes(uint32_t slots_per_xcd)
{
  return ((size_t)PT_PARK_XCDS * slots_per_xcd * sizeof(uint32_t) + 255) & ~(size_t)255;
}

/* -> the device's workspace (allocated and its flags zeroed at the first call), or nullptr when the allocation fails:
 * the scene then renders on the lane-waiting kernels, and rt_hip_kernel_name says so.  The current device is `device`. */
char *park_acquire_ws(int device, uint32_t *slots_per_xcd)
{
  if (device < 0 || device >= 64)
    return nullptr;
  if (g_fail_alloc.load() & RT_HIP_FAIL_ALLOC_PARK_WS) /* tests: behave as if the allocation had failed */
    return nullptr;
  std::lock_guard<std::mutex> lock(g_park_mutex);
  ParkPool &p = g_park[device];
  if (!p.ws)
  {
    const uint32_t per = pt_pool_slots_per_xcd(true);
    const size_t n_slots = (size_t)PT_PARK_XCDS * per;
    char *ws = nullptr;
    if (hipMalloc(&ws, park_flag_bytes(per) + n_slots * (PT_BLOCK / 64) * (size_t)PT_PARK_WAVE_BYTES) != hipSuccess)
    {
      (void)hipGetLastError();
      return nullptr;
    }
    /* the flags must be zero before a kernel on ANY stream looks at them (kernels leave them zero) */
    if (hipMemset(ws, 0, park_flag_bytes(per)) != hipSuccess || hipStreamSynchronize(nullptr) != hipSuccess)
    {
      (void)hipGetLastError();
      (void)hipFree(ws);
      return nullptr;
    }
    p.ws = ws;
    p.slots_per_xcd = per;
  }
  p.users++;
  *slots_per_xcd = p.slots_per_xcd;
  return p.ws;
}

/* a scene that held the device's workspace goes away (its launches have been waited for): the last one frees it */
void park_drop_ws(int device)
{
  if (device < 0 || device >= 64)
    return;
  std::lock_guard<std::mutex> lock(g_park_mutex);
  ParkPool &p = g_park[device];
  if (p.users > 0 && --p.users == 0)
  {
    (void)hipFree(p.ws);
    p.ws = nullptr;
    p.slots_per_xcd = 0;
  }
}

/* the per-device pool of pending-ray stacks of the two-child kernels (pt_scene_ctx.h, PendStack): flags, then
 * PT_PARK_XCDS x slots_per_xcd (pt_pool_slots_per_xcd: 160 on an MI355X) slots of `entries` x 10 fields x PT_PEND_COLUMNS doubles.  Sized by the deepest launch
 * seen so far (max_depth + 2 entries: 367 MB at the reference's MAX_DEPTH 5, 1.8 GB at the limit of 32); grown -- after
 * the device has drained -- when a launch needs more, never shrunk; rt_hip_release_cache() frees it. */
struct PendPool
{
  char *ws = nullptr;
  uint32_t entries = 0, columns = 0, slots_per_xcd = 0;
  uint32_t small_streak = 0; /* consecutive launches that needed at most a quarter of it (pend_pool_for: when it shrinks) */
};
/* a pool above PEND_SHRINK_ABOVE bytes is given up for one that fits after PEND_SHRINK_AFTER launches in a row needed at most a
 * quarter of it: one max_depth-29 glass-mesh launch used to pin 6.5 GB until rt_hip_release_cache() (round-4 advisor finding) */
constexpr size_t PEND_SHRINK_ABOVE = (size_t)1 << 30;
constexpr uint32_t PEND_SHRINK_AFTER = 16;
std::mutex g_pend_mutex; /* held from the pool lookup until the launch that uses it is enqueued (so that a growing
                          * launch's hipDeviceSynchronize covers every kernel that holds the old pointer) */
PendPool g_pend[64];

size_t pend_flag_bytes(uint32_t slots_per_xcd) { return ((size_t)PT_PARK_XCDS * slots_per_xcd * sizeof(uint32_t) + 255) & ~(size_t)255; }

/* caller holds g_pend_mutex; the current device is `device` */
int pend_pool_for(int device, uint32_t entries, uint32_t columns, PtLaunch &L)
{
  if (device < 0 || device >= 64)
    return fail(RT_HIP_ENODEV, "device %d: no pending-ray pool", device);
  PendPool &p = g_pend[device];
  if (p.ws && p.entries >= entries && p.columns >= columns)
  { /* large enough.  Far too large, for a while now?  Then the device drains once and the pool is rebuilt to fit. */
    const size_t have_bytes = (size_t)PT_PARK_XCDS * p.slots_per_xcd * p.entries * PT_PEND_FIELDS_HOST * p.columns * sizeof(double);
    if (have_bytes > PEND_SHRINK_ABOVE && (uint64_t)entries * columns * 4u <= (uint64_t)p.entries * p.columns)
    {
      if (++p.small_streak >= PEND_SHRINK_AFTER)
      {
        HIP_TRY(hipDeviceSynchronize());
        (void)hipFree(p.ws);
        p.ws = nullptr;
        p.entries = p.columns = p.small_streak = 0;
      }
    }
    else
      p.small_streak = 0;
  }
  if (p.entries < entries || p.columns < columns)
  {
    const bool asks_wide = columns > PT_PEND_COLUMNS && p.columns < columns; /* this launch is what asks for 4 x 512 stacks per slot */
    entries = std::max(entries, p.entries); /* grown in either direction, never shrunk */
    columns = std::max(columns, p.columns);
    const uint32_t per = p.slots_per_xcd ? p.slots_per_xcd : pt_pool_slots_per_xcd(false);
    const size_t slot_bytes = (size_t)entries * PT_PEND_FIELDS_HOST * columns * sizeof(double);
    const size_t n_slots = (size_t)PT_PARK_XCDS * per;
    /* tests: the request for 4 x 512 stacks per slot behaves as if hipMalloc had failed (BEFORE the old pool is given up) */
    if (asks_wide && (g_fail_alloc.load() & RT_HIP_FAIL_ALLOC_WIDE_PEND))
      return fail(RT_HIP_ENOMEM, "pending-ray pool for max_depth %u (%zu MB): allocation failure injected", entries - 2u,
                  (pend_flag_bytes(per) + n_slots * slot_bytes) >> 20);
    if (p.ws)
    {
      HIP_TRY(hipDeviceSynchronize());
      (void)hipFree(p.ws);
      p.ws = nullptr;
      p.entries = p.columns = 0;
    }
    char *ws = nullptr;
    hipError_t e = hipMalloc(&ws, pend_flag_bytes(per) + n_slots * slot_bytes);
    if (e != hipSuccess)
    {
      (void)hipGetLastError(); /* the caller may go on with a narrower pool: a later hipGetLastError() must not see this failure (round-4 advisor finding) */
      return fail(RT_HIP_ENOMEM, "pending-ray pool for max_depth %u (%zu MB): %s", entries - 2u,
                  (pend_flag_bytes(per) + n_slots * slot_bytes) >> 20, hipGetErrorString(e));
    }
    e = hipMemset(ws, 0, pend_flag_bytes(per));
    if (e == hipSuccess)
      e = hipStreamSynchronize(nullptr); /* the flags are zero before a kernel on any stream looks at them */
    if (e != hipSuccess)
    {
      (void)hipGetLastError();
      (void)hipFree(ws);
      return fail(RT_HIP_ERUNTIME, "pending-ray pool: %s", hipGetErrorString(e));
    }
    p.ws = ws;
    p.entries = entries;
    p.columns = columns;
    p.slots_per_xcd = per;
    p.small_streak = 0;
  }
  L.pend_flags = reinterpret_cast<uint32_t *>(p.ws);
  L.pend_ws = reinterpret_cast<double *>(p.ws + pend_flag_bytes(p.slots_per_xcd));
  L.pend_slots_per_xcd = p.slots_per_xcd;
  L.pend_entries = p.entries; /* slots are laid out for the pool's depth; a shallower launch uses a prefix of each */
  L.pend_slot_doubles = (uint64_t)p.entries * PT_PEND_FIELDS_HOST * p.columns;
  return RT_HIP_OK;
}

/* A pending-ray pool of an accumulation's own (rt_hip_accum_create): laid out as the device's pool (flags, then slots), allocated
 * once for the plan and held until rt_hip_accum_destroy, so that no other launch can grow, shrink or free it mid-frame.  The
 * injected failure of the wide pool applies as in pend_pool_for.  The current device is the scene's. */
int pend_pool_own(uint32_t entries, uint32_t columns, PtLaunch &L, DeviceBuffer &out)
{
  const uint32_t per = pt_pool_slots_per_xcd(false);
  const size_t slot_bytes = (size_t)entries * PT_PEND_FIELDS_HOST * columns * sizeof(double);
  const size_t bytes = pend_flag_bytes(per) + (size_t)PT_PARK_XCDS * per * slot_bytes;
  if (columns > PT_PEND_COLUMNS && (g_fail_alloc.load() & RT_HIP_FAIL_ALLOC_WIDE_PEND))
    return fail(RT_HIP_ENOMEM, "pending-ray pool for max_depth %u (%zu MB): allocation failure injected", entries - 2u, bytes >> 20);
  DeviceBuffer ws;
  hipError_t e = ws.alloc(bytes);
  if (e != hipSuccess)
    return fail(RT_HIP_ENOMEM, "pending-ray pool for max_depth %u (%zu MB): %s", entries - 2u, bytes >> 20, hipGetErrorString(e));
  e = hipMemset(ws.ptr, 0, pend_flag_bytes(per));
  if (e == hipSuccess)
    e = hipStreamSynchronize(nullptr);
  if (e != hipSuccess)
  {
    (void)hipGetLastError();
    return fail(RT_HIP_ERUNTIME, "pending-ray pool: %s", hipGetErrorString(e));
  }
  L.pend_flags = ws.at<uint32_t>();
  L.pend_ws = ws.at<double>(pend_flag_bytes(per));
  L.pend_slots_per_xcd = per;
  L.pend_entries = entries;
  L.pend_slot_doubles = (uint64_t)entries * PT_PEND_FIELDS_HOST * columns;
  out = std::move(ws);
  return RT_HIP_OK;
}

/* the per-device status word of render launches (PtLaunch.status, rt_hip_launch_status) */
std::mutex g_status_mutex;
uint32_t *g_status[64] = {nullptr};

/* the current device is `device` */
int status_word_for(int device, uint32_t **out)
{
  if (device < 0 || device >= 64)
    return fail(RT_HIP_ENODEV, "device %d: no status word", device);
  std::lock_guard<std::mutex> lock(g_status_mutex);
  if (!g_status[device])
  {
    uint32_t *w = nullptr;
    HIP_TRY(hipMalloc(&w, 256));
    hipError_t e = hipMemset(w, 0, 256);
    if (e == hipSuccess)
      e = hipStreamSynchronize(nullptr);
    if (e != hipSuccess)
    {
      (void)hipFree(w);
      return fail(RT_HIP_ERUNTIME, "status word: %s", hipGetErrorString(e));
    }
    g_status[device] = w;
  }
  *out = g_status[device];
  return RT_HIP_OK;
}

/* reads and clears the device's status word; the current device is `device` */
int status_take(int device, uint32_t *flags)
{
  *flags = 0;
  uint32_t *w = nullptr;
  {
    std::lock_guard<std::mutex> lock(g_status_mutex);
    w = (device >= 0 && device < 64) ? g_status[device] : nullptr;
  }
  if (!w)
    return RT_HIP_OK; /* nothing has been launched on this device */
  HIP_TRY(hipMemcpy(flags, w, sizeof *flags, hipMemcpyDeviceToHost));
  if (*flags)
    HIP_TRY(hipMemset(w, 0, sizeof *flags));
  return RT_HIP_OK;
}

int status_to_error(uint32_t flags)
{
  if (!flags)
    return RT_HIP_OK;
  return fail(RT_HIP_ERUNTIME, "render launch failed on the device:%s%s -- the affected tiles were not rendered (they read NaN / 255)",
              (flags & RT_HIP_FAIL_PEND_SLOT) ? " a workgroup found no free slot in the pending-ray pool;" : "",
              (flags & RT_HIP_FAIL_PARK_SLOT) ? " a workgroup found no free slot in the parked-walk workspace;" : "");
}

void pend_pools_release()
{
  std::lock_guard<std::mutex> lock(g_pend_mutex);
  int prev = 0;
  (void)hipGetDevice(&prev);
  for (int d = 0; d < 64; d++)
    if (g_pend[d].ws)
    {
      (void)hipSetDevice(d);
      (void)hipDeviceSynchronize();
      (void)hipFree(g_pend[d].ws);
      g_pend[d] = PendPool();
    }
  {
    std::lock_guard<std::mutex> slock(g_status_mutex);
    for (int d = 0; d < 64; d++)
      if (g_status[d])
      {
        (void)hipSetDevice(d);
        (void)hipDeviceSynchronize();
        (void)hipFree(g_status[d]);
        g_status[d] = nullptr;
      }
  }
  (void)hipSetDevice(prev);
}

/* ---- the mixed grid (PtLaunch.n_whole): a one-chunk launch of many rounds of workgroups ends with the device
 * partly empty -- the dispatcher runs dry while every CU still holds workgroups at random points of their lives, and the frame ends
 * with the last of them.  So the launch's LAST tiles run as sample chunks, short workgroups, behind the whole ones: one launch, the
 * same sums bit for bit (integer partial sums, pt_resolve_tiles), and only those tiles pay the chunks' prologues and the resolve.
 * The shim chooses it by itself where the caller asked for one chunk and gave no workspace; the chunked slots' records live in a
 * per-device workspace the shim owns (GridTailWs), as the parked-walk workspace is owned. */
struct GridTailWs
{
  unsigned long long *ws = nullptr; /* a raw pointer, as the other per-device pools hold theirs: freed by grid_tail_release() alone, never at exit */
  size_t bytes = 0;
  hipEvent_t done = nullptr;   /* recorded behind the last launch that used the workspace ... */
  hipStream_t stream = nullptr; /* ... on this stream: a launch on another stream waits for it first */
  bool used = false;
  /* what pt_resident_workgroups said last on this device, and for which member and dynamic LDS: asked again only when those change */
  uint32_t resident = 0;
  int resident_kernel = -1;
  size_t resident_lds = 0;
};
std::mutex g_tail_mutex; /* held from the lookup until the launch that uses the workspace is enqueued */
GridTailWs g_tail[64];
std::atomic<uint64_t> g_mixed_launches{0};

/* The rule.  It reads launch facts only: the slots, the samples, the workgroups the device holds at once (pt_resident_workgroups:
 * 1,280 of pt_render_tiles on an MI355X).  A launch of fewer than GRID_TAIL_MIN_ROUNDS rounds of workgroups stays as it is -- there
 * the chunks' prologues weigh more and the tail is a larger share of a frame that suggest_chunks already covers --, and a chunk keeps
 * at least GRID_TAIL_MIN_SAMPLES samples (rt_hip_suggest_chunks' floor).  The last GRID_TAIL_ROUNDS rounds' worth of slots are
 * chunked, GRID_TAIL_CHUNKS workgroups each: swept on the headline, profiles/r20_grid_tail_sweep.txt.  GRID_TAIL_MIN_ROUNDS is NOT
 * measured: the headline's 25 rounds are the only launch length timed, and 8 is a guess that keeps a third of that.
 * Two switches for A/B runs and tests, read at every launch: RT_HIP_GRID_UNIFORM=1 keeps every launch uniform;
 * RT_HIP_GRID_SPLIT=<n_whole>,<chunks> sets the split of every launch whose FORM takes one (one chunk asked, no workspace given, a
 * MIXED member, a plain one-shot launch) whatever its size: n_whole >= the slots is the uniform one-chunk launch, 0 the uniform
 * chunked one. */
constexpr uint32_t GRID_TAIL_MIN_ROUNDS = 8, GRID_TAIL_ROUNDS = 1, GRID_TAIL_CHUNKS = 4, GRID_TAIL_MIN_SAMPLES = 128;

/* -> true with *n_whole, *chunks set: the launch takes them (n_whole < tile_count, chunks >= 2); false: it stays uniform */
bool grid_split_for(const PtLaunch &L, const PtPlan &plan, int device, uint32_t *n_whole, uint32_t *chunks)
{
  if (!plan.mixed || plan.sample_chunks != 1u || L.acc_keep || L.slot_list || L.tile_count < 2u || L.samples < 2)
    return false;
  const char *uni = getenv("RT_HIP_GRID_UNIFORM");
  if (uni && uni[0] == '1')
    return false;
  if (const char *e = getenv("RT_HIP_GRID_SPLIT"))
  {
    char *end = nullptr;
    const unsigned long w = strtoul(e, &end, 10);
    const unsigned long c = (end && *end == ',') ? strtoul(end + 1, nullptr, 10) : 0ul;
    if (w >= L.tile_count || c < 2ul || c > (unsigned long)L.samples || (uint64_t)(L.tile_count - w) * c + w > 0x7FFFFFFFull)
      return false;
    *n_whole = (uint32_t)w;
    *chunks = (uint32_t)c;
    return true;
  }
  /* the free tests first: a launch of few samples or few tiles asks the runtime nothing and takes no lock */
  if ((uint32_t)L.samples < GRID_TAIL_CHUNKS * GRID_TAIL_MIN_SAMPLES || L.tile_count < GRID_TAIL_MIN_ROUNDS || device < 0 || device >= 64)
    return false;
  uint32_t resident = 0;
  {
    std::lock_guard<std::mutex> lock(g_tail_mutex);
    GridTailWs &t = g_tail[device];
    const size_t lds = pt_render_lds_bytes(L.scene);
    if (t.resident_kernel != plan.kernel || t.resident_lds != lds)
    {
      t.resident = pt_resident_workgroups(plan.kernel, L.scene);
      t.resident_kernel = plan.kernel;
      t.resident_lds = lds;
    }
    resident = t.resident;
  }
  if (resident == 0u || (uint64_t)L.tile_count < (uint64_t)GRID_TAIL_MIN_ROUNDS * resident)
    return false;
  *n_whole = L.tile_count - GRID_TAIL_ROUNDS * resident;
  *chunks = GRID_TAIL_CHUNKS;
  return true;
}

/* The device's workspace for n_chunked slots, grown when a launch needs more (after the device has drained), and `stream` made to
 * wait for the launch that used it last where that ran elsewhere.  nullptr: it cannot be had (or RT_HIP_FAIL_ALLOC_TAIL_WS says
 * so), and the launch stays uniform.  The caller holds g_tail_mutex, the current device is `device`; grid_tail_used() follows the launch. */
unsigned long long *grid_tail_ws(int device, uint32_t n_chunked, hipStream_t stream)
{
  if (device < 0 || device >= 64 || (g_fail_alloc.load() & RT_HIP_FAIL_ALLOC_TAIL_WS))
    return nullptr;
  GridTailWs &t = g_tail[device];
  const size_t need = (size_t)n_chunked * PT_ACC_WS_WORDS * sizeof(unsigned long long);
  if (t.bytes < need)
  {
    if (t.ws)
    {
      if (hipDeviceSynchronize() != hipSuccess)
      {
        (void)hipGetLastError();
        return nullptr;
      }
      (void)hipFree(t.ws);
      t.ws = nullptr;
    }
    t.bytes = 0;
    t.used = false;
    if (hipMalloc(&t.ws, need) != hipSuccess)
    {
      (void)hipGetLastError(); /* the launch goes on uniform: nothing sticky behind the failure */
      t.ws = nullptr;
      return nullptr;
    }
    t.bytes = need;
  }
  if (!t.done && hipEventCreateWithFlags(&t.done, hipEventDisableTiming) != hipSuccess)
  {
    (void)hipGetLastError();
    t.done = nullptr;
    return nullptr;
  }
  if (t.used && t.stream != stream && hipStreamWaitEvent(stream, t.done, 0) != hipSuccess)
  {
    (void)hipGetLastError();
    return nullptr;
  }
  return t.ws;
}

void grid_tail_used(int device, hipStream_t stream)
{
  GridTailWs &t = g_tail[device];
  if (hipEventRecord(t.done, stream) != hipSuccess)
  { /* nothing to order the next user by: let this one finish */
    (void)hipGetLastError();
    (void)hipStreamSynchronize(stream);
    t.used = false;
    return;
  }
  t.stream = stream;
  t.used = true;
}

void grid_tail_release()
{
  std::lock_guard<std::mutex> lock(g_tail_mutex);
  int prev = 0;
  (void)hipGetDevice(&prev);
  for (int d = 0; d < 64; d++)
    if (g_tail[d].ws || g_tail[d].done)
    {
      (void)hipSetDevice(d);
      (void)hipDeviceSynchronize();
      if (g_tail[d].done)
        (void)hipEventDestroy(g_tail[d].done);
      if (g_tail[d].ws)
        (void)hipFree(g_tail[d].ws);
      g_tail[d] = GridTailWs();
    }
  (void)hipSetDevice(prev);
}

uint32_t tiles_x_of(int width) { return ((uint32_t)width + PT_TILE - 1) / PT_TILE; }
uint32_t tiles_y_of(int height) { return ((uint32_t)height + PT_TILE - 1) / PT_TILE; }

int check_params(const RtHipParams *p)
{
  if (!p)
    return fail(RT_HIP_EINVAL, "params is NULL");
  if (p->width < 2 || p->height < 2)
    return fail(RT_HIP_EINVAL, "width and height must be >= 2 (the reference divides by width-1, height-1)");
  if (p->samples < 1 || p->samples > (1 << 26))
    return fail(RT_HIP_EINVAL, "samples must be in [1, 2^26]");
  if (p->max_depth < 0 || p->max_depth > 1000000)
    return fail(RT_HIP_EINVAL, "max_depth out of range");
  if (p->integrator != RT_HIP_TRACE_PATH && p->integrator != RT_HIP_CAST_RAY)
    return fail(RT_HIP_EINVAL, "integrator must be RT_HIP_TRACE_PATH (0) or RT_HIP_CAST_RAY (1)");
  if ((uint64_t)p->width * (uint64_t)p->height > 0xFFFFFFFFull)
    return fail(RT_HIP_EINVAL, "image has more than 2^32 pixels");
  if (p->width > (1 << 20) || p->height > (1 << 20))
    return fail(RT_HIP_EINVAL, "width and height must not exceed 2^20 (the kernel's exact-quotient shortcut)");
  return RT_HIP_OK;
}

/* every tile of the image, in order */
void whole_image(RtHipParams &p)
{
  p.tile_first = 0;
  p.tile_stride = 1;
  p.tile_count = tiles_x_of(p.width) * tiles_y_of(p.height);
}

int check_adapt(const RtHipAdaptParams *p)
{
  if (p->min_samples < 1 || p->dilate > 2u || p->threshold != p->threshold)
    return fail(RT_HIP_EINVAL, "adaptive parameters: min_samples >= 1, dilate 0 .. 2, threshold not NaN");
  return RT_HIP_OK;
}

/* the scalars of bvh_build.h into the scene -- at creation, and after every update of the spheres (`reach` is the caller's) */
void take_sphere_bounds(RtHipScene *sc, const SceneSphereBounds &sb)
{
  sc->view.wide_range = (sb.wide_range || sc->force_wide) ? 1u : 0u;
  sc->max_center = sb.max_center;
  sc->n_big = (int)sb.n_big;
  for (int k = 0; k < SCENE_SPHERE_WALLS; k++)
  {
    sc->big_r[k] = sb.big_r[k];
    sc->big_c[k] = sb.big_c[k];
  }
  sc->reach_spheres = sb.reach_spheres;
}

/* its twin for the triangles -- at creation, and after every update of the vertices */
void take_mesh_bounds(RtHipScene *sc, const SceneMeshBounds &mb)
{
  for (int a = 0; a < 3; a++)
    sc->mesh_c[a] = mb.c[a];
  sc->mesh_R = mb.R;
  sc->mesh_c_norm = mb.c_norm;
  sc->view.mesh_round = mb.round ? 1u : 0u;
}

/* ... and for the materials -- at creation, and after every update of the materials */
void take_material_bounds(RtHipScene *sc, const SceneMaterialBounds &b)
{
  sc->max_emission = b.max_emission;
  sc->view.any_refract = (b.classes & SCENE_MATERIAL_REFRACT) ? 1u : 0u;
  sc->view.any_checker = (b.classes & SCENE_MATERIAL_CHECKER) ? 1u : 0u;
  sc->any_mirror_glass = (b.classes & SCENE_MATERIAL_MIRROR_GLASS) != 0;
  sc->view.any_mirror_glass = sc->any_mirror_glass ? 1u : 0u;
}

/* hull facets (pt_build_hull_flags) with the margin scene_mesh_bounds gave, where there is one and the triangles are few enough;
 * tri_object's bits are clear before.  Enqueues on the null stream: the caller waits. */
hipError_t scene_hull_flags(RtHipScene *sc, double tau)
{
  const uint32_t n = sc->view.n_triangles;
  sc->hull_flags = false;
  if (n == 0 || n > PT_HULL_MAX_TRIS || tau < 0)
    return hipSuccess;
  const hipError_t e =
      pt_launch_build_hull_flags(sc->view.tri_geom, sc->view.tri_normal, n, tau, const_cast<uint32_t *>(sc->view.tri_object), nullptr);
  sc->hull_flags = e == hipSuccess;
  return e;
}

/* the device builder over tri_geom (device memory, n x 9) with the refusals that creation and rebuild share */
int build_device_tree(const double *tri_geom, size_t n, BvhDeviceTree *tree)
{
  const hipError_t be = bvh_device_build(tri_geom, (uint32_t)n, tree);
  if (be != hipSuccess && tree->failure)
    return fail(RT_HIP_ERUNTIME, "device hierarchy builder: %s", tree->failure);
  HIP_TRY(be);
  if (tree->depth > PT_BVH_STACK)
    return fail(RT_HIP_ELIMIT, "triangle hierarchy depth %d exceeds the traversal stack (%d)", tree->depth, PT_BVH_STACK);
  if (tree->n_nodes == 0)
    return fail(RT_HIP_ERUNTIME, "device hierarchy builder: a tree without nodes");
  return RT_HIP_OK;
}

/* A device-built tree into the scene: nodes and order out of the builder's workspace to where view.bvh_src and view.bvh_tri point
 * (room for tree.n_nodes is the caller's business), the leaf-ordered geometry gathered from view.tri_geom, a wait for the null
 * stream, then the scalars that describe the tree. */
hipError_t install_device_tree(RtHipScene *sc, const BvhDeviceTree &tree)
{
  const uint32_t n = sc->view.n_triangles;
  hipError_t e = hipMemcpy(const_cast<double *>(sc->view.bvh_src), tree.nodes, (size_t)tree.n_nodes * PT_BVH_SRC_DOUBLES * 8, hipMemcpyDeviceToDevice);
  if (e == hipSuccess)
    e = hipMemcpy(const_cast<uint32_t *>(sc->view.bvh_tri), tree.order, (size_t)n * 4, hipMemcpyDeviceToDevice);
  if (e == hipSuccess)
    e = bvh_device_gather_leaf(sc->view.tri_geom, sc->view.bvh_tri, n, const_cast<double *>(sc->view.tri_geom_leaf));
  if (e == hipSuccess)
    e = hipStreamSynchronize(nullptr);
  if (e != hipSuccess)
    return e;
  sc->view.n_bvh_nodes = tree.n_nodes;
  sc->view.bvh_depth = (uint32_t)tree.depth;
  sc->bvh_builder = RT_HIP_BVH_DEVICE;
  sc->bvh_max_depth = (uint32_t)tree.max_depth;
  sc->bvh_build_seconds = 1e-3 * tree.build_ms;
  sc->bvh_nodes_bytes = (size_t)tree.n_nodes * PT_BVH_NODE_WORDS * 4;
  return hipSuccess;
}

int scene_create_impl(const RtHipSphere *spheres, size_t n_spheres, const RtHipMesh *meshes, size_t n_meshes,
                      int device, uint32_t bvh_builder, RtHipScene **out_scene)
{
  if (!out_scene)
    return fail(RT_HIP_EINVAL, "out_scene is NULL");
  *out_scene = nullptr;
  if ((n_spheres && !spheres) || (n_meshes && !meshes))
    return fail(RT_HIP_EINVAL, "NULL scene array with non-zero count");
  if (!have_device(device))
    return fail(RT_HIP_ENODEV, "no HIP device %d (found %d)", device, usable_devices());

  size_t n_tri = 0;
  for (size_t i = 0; i < n_spheres; i++)
  {
    if (!scene_material_ok(spheres[i].color, spheres[i].emission))
      return fail(RT_HIP_EINVAL, "sphere %zu: colour must be finite and >= 0, emission finite", i);
    if (!scene_sphere_radius_ok(spheres[i].radius))
      return fail(RT_HIP_ELIMIT, "sphere %zu: |radius| %g outside [1e-100, 1e100]", i, spheres[i].radius);
  }
  for (size_t m = 0; m < n_meshes; m++)
  {
    if (!scene_material_ok(meshes[m].color, meshes[m].emission))
      return fail(RT_HIP_EINVAL, "mesh %zu: colour must be finite and >= 0, emission finite", m);
    if (meshes[m].num_triangles && !meshes[m].vertices)
      return fail(RT_HIP_EINVAL, "mesh %zu has triangles but no vertices", m);
    n_tri += meshes[m].num_triangles;
  }
  if (n_spheres + n_meshes > 0xFFFFFFu || n_tri > 0x7FFFFFFFu - n_spheres)
    return fail(RT_HIP_ELIMIT, "scene too large");
  const size_t n_mat = n_spheres + n_meshes;

  /* ---- build the kernel layout on the host (pt_device.h) ---- */
  double reach = 0, reach_triangles = 0;
  std::vector<double> geom(PT_ENTRY_SRC_STRIDE * (n_spheres + n_tri)), mat(PT_MAT_STRIDE * n_mat), tgeom(9 * n_tri), tnorm(3 * n_tri),
      ttex(6 * n_tri);
  std::vector<uint32_t> tobj(n_tri);
  std::vector<double> craw(3 * n_mat), geom4(PT_GEOM_STRIDE * n_spheres);
  /* the materials' records and what the scene derives from them: bvh_build.h, as an update of the materials derives it again */
  SceneMaterialBounds matb;
  {
    std::vector<double> in(SCENE_MATERIAL_IN * n_mat);
    std::vector<uint32_t> flags(n_mat);
    for (size_t i = 0; i < n_mat; i++)
    {
      const bool sph = i < n_spheres;
      memcpy(&in[SCENE_MATERIAL_IN * i], sph ? spheres[i].color : meshes[i - n_spheres].color, 3 * sizeof(double));
      memcpy(&in[SCENE_MATERIAL_IN * i + 3], sph ? spheres[i].emission : meshes[i - n_spheres].emission, 3 * sizeof(double));
      flags[i] = sph ? spheres[i].flags : meshes[i - n_spheres].flags;
    }
    scene_material_bounds(in.data(), flags.data(), n_mat, mat.data(), craw.data(), &matb);
  }
  /* the spheres' records and what the scene derives from them: bvh_build.h, as an update of the spheres derives it again */
  SceneSphereBounds sb;
  {
    std::vector<double> in(SCENE_SPHERE_IN * n_spheres);
    for (size_t i = 0; i < n_spheres; i++)
    {
      memcpy(&in[SCENE_SPHERE_IN * i], spheres[i].center, 3 * sizeof(double));
      in[SCENE_SPHERE_IN * i + 3] = spheres[i].radius;
    }
    scene_sphere_bounds(in.data(), n_spheres, geom.data(), geom4.data(), &sb);
  }
  reach = sb.reach_spheres;
  size_t t = 0;
  for (size_t m = 0; m < n_meshes; m++)
    for (size_t k = 0; k < 3 * meshes[m].num_triangles; k++)
    {
      const double *q = meshes[m].vertices[k].pos;
      const double len = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]);
      /* a non-finite coordinate is refused here: fmax(reach, NaN) would drop it silently, the hierarchy builder would sort
       * NaN centroids (no strict weak ordering) and quantise them (undefined), and the kernels' UNSCALED division would lose
       * its range argument (round-4 advisor finding).  The reference has no such check -- and no meaning for such a triangle:
       * every comparison of its test (raytracer.c:137-150) is false or the triangle is never hit. */
      if (!(len <= 1e300))
        return fail(RT_HIP_EINVAL, "mesh %zu: vertex %zu has a non-finite coordinate", m, k);
      /* (a vertex far out needs no flag of its own: it is part of `reach`, and a launch refuses
       * near_R = 1.5 (|camera| + reach) + 1 >= 1e15 as "not a usable finite bound" -- so every vertex a kernel ever sees
       * lies within 6.7e14 of the origin, which is what exact_triangle's UNSCALED division rests on, see below) */
      reach = std::fmax(reach, len);
      reach_triangles = std::fmax(reach_triangles, len);
    }
  for (size_t m = 0; m < n_meshes; m++)
  {
    for (size_t k = 0; k < meshes[m].num_triangles; k++, t++)
    {
      const RtHipVertex *v = meshes[m].vertices + 3 * k;
      double *g = &tgeom[9 * t];
      scene_triangle_entry(v[0].pos, v[1].pos, v[2].pos, g, &geom[PT_ENTRY_SRC_STRIDE * (n_spheres + t)]);
      scene_triangle_normal(g, &tnorm[3 * t]);
      for (int j = 0; j < 3; j++)
      {
        ttex[6 * t + 2 * j + 0] = v[j].tex[0];
        ttex[6 * t + 2 * j + 1] = v[j].tex[1];
      }
      tobj[t] = (uint32_t)(n_spheres + m);
    }
  }

  /* ---- bounding sphere of all triangles, as the kernels see them (v0, v0 + e1, v0 + e2): the two reductions here, what follows
   * them in bvh_build.h's one text, as an update of the vertices derives it again ---- */
  SceneMeshBounds mb;
  if (n_tri != 0)
  {
    double lo[3] = {HUGE_VAL, HUGE_VAL, HUGE_VAL}, hi[3] = {-HUGE_VAL, -HUGE_VAL, -HUGE_VAL}, c[3], p[3], r2 = 0;
    for (size_t i = 0; i < 3 * n_tri; i++)
    {
      scene_triangle_corner(&tgeom[9 * (i / 3)], (int)(i % 3), p);
      for (int a = 0; a < 3; a++)
      {
        lo[a] = std::fmin(lo[a], p[a]);
        hi[a] = std::fmax(hi[a], p[a]);
      }
    }
    scene_mesh_centre(lo, hi, c);
    for (size_t i = 0; i < 3 * n_tri; i++)
    {
      scene_triangle_corner(&tgeom[9 * (i / 3)], (int)(i % 3), p);
      const double dx = p[0] - c[0], dy = p[1] - c[1], dz = p[2] - c[2];
      r2 = std::fmax(r2, dx * dx + dy * dy + dz * dz);
    }
    scene_mesh_bounds(lo, hi, r2, &mb);
  }

  /* ---- hierarchy over the triangles ---- */
  BvhBuild bvh;
  /* RT_HIP_BVH_DEVICE: the tree stays in the build's workspace, and the triangles it was built from in `dgeom`, until the blob --
   * sized by the node count the build produces -- has taken both, device to device */
  BvhDeviceTree dtree;
  DeviceBuffer dgeom;
  size_t n_bvh_nodes = 0;
  int bvh_depth = 0, bvh_max_depth = 0;
  double bvh_build_seconds = 0;
  /* built for every scene with triangles: the small-scene kernels scan them through the flat
   * filter instead, but the general in-memory kernels (too-large scenes, cast_ray with
   * two-child materials) always walk the hierarchy */
  if (n_tri > 0)
  {
    if (n_tri >= (1u << (31 - PT_BVH_COUNT_BITS)))
      return fail(RT_HIP_ELIMIT, "%zu triangles exceed the hierarchy's leaf references (2^%d)", n_tri, 31 - PT_BVH_COUNT_BITS);
    if (bvh_builder == RT_HIP_BVH_DEVICE)
    {
      DeviceScope build_scope(device);
      HIP_TRY(build_scope.status);
      HIP_TRY(dgeom.alloc(tgeom.size() * 8));
      HIP_TRY(hipMemcpy(dgeom.ptr, tgeom.data(), tgeom.size() * 8, hipMemcpyHostToDevice));
      const int rc = build_device_tree(dgeom.at<double>(), n_tri, &dtree);
      if (rc)
        return rc;
      n_bvh_nodes = dtree.n_nodes; /* the blob is sized by it; install_device_tree gives the scene the rest */
    }
    else
    {
      const auto t0 = std::chrono::steady_clock::now();
      bvh.tgeom = tgeom.data();
      bvh.order.resize(n_tri);
      bvh.cen.resize(3 * n_tri);
      bvh.lo.resize(3 * n_tri);
      bvh.hi.resize(3 * n_tri);
      for (uint32_t k = 0; k < (uint32_t)n_tri; k++)
      {
        bvh.order[k] = k;
        bvh.tri_box(k);
      }
      bvh.build_root((uint32_t)n_tri);
      n_bvh_nodes = bvh.nodes.size() / PT_BVH_SRC_DOUBLES;
      bvh_depth = bvh.depth;
      bvh_max_depth = bvh.max_depth;
      bvh_build_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
      if (bvh_depth > PT_BVH_STACK)
        return fail(RT_HIP_ELIMIT, "triangle hierarchy depth %d exceeds the traversal stack (%d)", bvh_depth, PT_BVH_STACK);
    }
  }
  std::vector<double> tgeom_leaf(9 * bvh.order.size()); /* host builder only: the device builder gathers on the device */
  for (size_t k = 0; k < bvh.order.size(); k++)
    memcpy(&tgeom_leaf[9 * k], &tgeom[9 * (size_t)bvh.order[k]], 9 * sizeof(double));

  /* ---- one device blob ---- */
  const size_t off_geom = 0;
  const size_t off_mat = off_geom + pad256(geom.size() * 8);
  const size_t off_craw = off_mat + pad256(mat.size() * 8);
  const size_t off_geom4 = off_craw + pad256(craw.size() * 8);
  const size_t off_tgeom = off_geom4 + pad256(geom4.size() * 8);
  const size_t off_tnorm = off_tgeom + pad256(tgeom.size() * 8);
  const size_t off_ttex = off_tnorm + pad256(tnorm.size() * 8);
  const size_t off_tobj = off_ttex + pad256(ttex.size() * 8);
  const size_t off_filt = off_tobj + pad256(tobj.size() * 4);
  /* + 1 pair: the scan's software pipeline reads one pair past the end */
  const size_t filt_bytes = pt_filt_bytes((uint32_t)n_spheres, (uint32_t)n_tri);
  const size_t off_bvh_src = off_filt + pad256(filt_bytes);
  const size_t off_bvh_nodes = off_bvh_src + pad256(n_bvh_nodes * PT_BVH_SRC_DOUBLES * 8);
  const size_t bvh_nodes_bytes = n_bvh_nodes * PT_BVH_NODE_WORDS * 4;
  const size_t off_bvh_tri = off_bvh_nodes + pad256(bvh_nodes_bytes);
  const size_t off_tgeom_leaf = off_bvh_tri + pad256(n_tri * 4);
  const size_t total = off_tgeom_leaf + pad256(9 * n_tri * 8) + 256;

  DeviceScope scope(device);
  HIP_TRY(scope.status);
  RtHipScene *sc = new (std::nothrow) RtHipScene;
  if (!sc)
    return fail(RT_HIP_ENOMEM, "host allocation failed");
  sc->device = device;
  hipError_t e = hipMalloc(&sc->blob, total);
  if (e != hipSuccess)
  {
    delete sc;
    return fail(RT_HIP_ENOMEM, "hipMalloc(%zu): %s", total, hipGetErrorString(e));
  }
  char *base = static_cast<char *>(sc->blob);
  sc->view.bvh_src = reinterpret_cast<const double *>(base + off_bvh_src);
  sc->view.bvh_tri = reinterpret_cast<const uint32_t *>(base + off_bvh_tri);
  sc->view.tri_geom_leaf = reinterpret_cast<const double *>(base + off_tgeom_leaf);
  sc->view.tri_geom = reinterpret_cast<const double *>(base + off_tgeom);
  sc->view.n_triangles = (uint32_t)n_tri;
  auto up = [&](size_t off, const void *src, size_t bytes) -> hipError_t {
    return bytes ? hipMemcpy(base + off, src, bytes, hipMemcpyHostToDevice) : hipSuccess;
  };
  e = up(off_geom, geom.data(), geom.size() * 8);
  if (e == hipSuccess) e = up(off_mat, mat.data(), mat.size() * 8);
  if (e == hipSuccess) e = up(off_craw, craw.data(), craw.size() * 8);
  if (e == hipSuccess) e = up(off_geom4, geom4.data(), geom4.size() * 8);
  if (e == hipSuccess)
    e = dgeom ? hipMemcpy(base + off_tgeom, dgeom.ptr, tgeom.size() * 8, hipMemcpyDeviceToDevice) : up(off_tgeom, tgeom.data(), tgeom.size() * 8);
  if (e == hipSuccess) e = up(off_tnorm, tnorm.data(), tnorm.size() * 8);
  if (e == hipSuccess) e = up(off_ttex, ttex.data(), ttex.size() * 8);
  if (e == hipSuccess) e = up(off_tobj, tobj.data(), tobj.size() * 4);
  if (e == hipSuccess) e = up(off_bvh_src, bvh.nodes.data(), bvh.nodes.size() * 8);
  if (e == hipSuccess) e = up(off_bvh_tri, bvh.order.data(), bvh.order.size() * 4);
  if (e == hipSuccess) e = up(off_tgeom_leaf, tgeom_leaf.data(), tgeom_leaf.size() * 8);
  sc->view.n_bvh_nodes = (uint32_t)n_bvh_nodes;
  sc->view.bvh_depth = (uint32_t)bvh_depth;
  sc->bvh_builder = bvh_builder;
  sc->bvh_max_depth = (uint32_t)bvh_max_depth;
  sc->bvh_build_seconds = bvh_build_seconds;
  if (e == hipSuccess && dtree.workspace)
    e = install_device_tree(sc, dtree);
  if (e != hipSuccess)
  {
    (void)hipFree(sc->blob);
    delete sc;
    return fail(RT_HIP_ERUNTIME, "scene upload: %s", hipGetErrorString(e));
  }
  sc->view.entry_src = reinterpret_cast<const double *>(base + off_geom);
  sc->view.filt = reinterpret_cast<float *>(base + off_filt);
  sc->view.bvh_nodes = reinterpret_cast<float *>(base + off_bvh_nodes);
  take_mesh_bounds(sc, mb);
  sc->filt_bytes = filt_bytes;
  sc->bvh_nodes_bytes = bvh_nodes_bytes;
  sc->bvh_node_capacity = (uint32_t)n_bvh_nodes;
  sc->view.material = reinterpret_cast<const double *>(base + off_mat);
  sc->view.color_raw = reinterpret_cast<const double *>(base + off_craw);
  sc->view.geom4 = reinterpret_cast<const double *>(base + off_geom4);
  sc->view.tri_normal = reinterpret_cast<const double *>(base + off_tnorm);
  sc->view.tri_tex = reinterpret_cast<const double *>(base + off_ttex);
  sc->view.tri_object = reinterpret_cast<const uint32_t *>(base + off_tobj);
  {
    hipError_t he = scene_hull_flags(sc, mb.tau);
    if (he == hipSuccess && sc->hull_flags)
      he = hipDeviceSynchronize();
    if (he != hipSuccess)
    {
      (void)hipFree(sc->blob);
      delete sc;
      return fail(RT_HIP_ERUNTIME, "hull flags: %s", hipGetErrorString(he));
    }
  }
  sc->view.n_spheres = (uint32_t)n_spheres;
  sc->view.n_meshes = (uint32_t)n_meshes;
#ifdef PT_DEV_KERNELS
  {
    /* development knob (tools/many_spheres.py): RT_HIP_FORCE_BIG=1 sends a small scene to the scalar-table _big kernels,
     * which it otherwise reaches only through a centre or radius beyond 1e17 */
    const char *fb = getenv("RT_HIP_FORCE_BIG");
    sc->force_wide = fb && fb[0] == '1';
  }
#endif
  take_sphere_bounds(sc, sb);
  sc->reach = reach;
  sc->reach_triangles = reach_triangles;
  sc->blob_bytes = total;
  take_material_bounds(sc, matb);
  *out_scene = sc;
  return RT_HIP_OK;
}

/* the scene has the parked-walk workspace, or would get it at its first launch (rt_hip_render_tiles_chunked acquires it) */
bool park_ws_expected(const RtHipScene *scene)
{
  std::lock_guard<std::mutex> lock(scene->table_mutex);
  /* (a scene that has met its workspace keeps it, whatever is injected later; one that has not yet would not get it now) */
  return scene->park_tried ? scene->park_ws != nullptr : (g_fail_alloc.load() & RT_HIP_FAIL_ALLOC_PARK_WS) == 0;
}

/* bvh_probe's bounding sphere of the triangles for one near_R: the thresholds of a bounding entry of the flat
 * filter in its compare form, widened exactly as pt_build_filter widens them (e = 2^-24, A = |c| + near_R:
 * |tca32 - tca| <= 6.2 e A, |d2_32 - d2| <= 20.5 e A^2 for origins within near_R; the conversions to fp32 are
 * inside the (1 + k e) factors).  Non-finite or overflowing values give thresholds that keep every ray. */
void mesh_bound_for(const RtHipScene *scene, double near_R, float out[5])
{
  const float inf = std::numeric_limits<float>::infinity();
  out[0] = out[1] = out[2] = 0.f;
  out[3] = inf;
  out[4] = -inf;
  if (!(scene->mesh_R >= 0) || !(scene->mesh_R < 1e18) || !(scene->mesh_c_norm < 1e18) || !(near_R < 1e18))
    return;
  const double e = 5.9604644775390625e-08, A = scene->mesh_c_norm + near_R;
  for (int a = 0; a < 3; a++)
    out[a] = (float)scene->mesh_c[a];
  out[3] = (float)((scene->mesh_R * scene->mesh_R + 32.0 * e * A * A) * (1.0 + 8.0 * e));
  out[4] = -(float)((scene->mesh_R + 10.0 * e * A) * (1.0 + 4.0 * e));
}

/* BigPrune (pt_filter.h, where the bounds are derived): for one near_R, the distance margin delta, the least estimate tmin
 * and per sphere the least q32 of a leading wall-sized sphere that may prune the others.  With e = 2^-24, A = |c| + near_R +
 * tol, W >= r2_hi' - r^2 (pt_sign_widen_total of pt_device.h, the very function pt_build_filter widens by, x 1.001), E = 28 e A^2 + 6 e | |c|^2 -
 * r^2 |:  qmin = (r / 16)^2 + W + E,  tmin = 2 (tol + 11.2 e A),  delta = 1.5 max (22.4 e A + 8 (W + E) / r).
 * Anything non-finite or implausible switches the pruning off. */
void big_prune_for(const RtHipScene *scene, double near_R, double filt_shift, PtLaunch &L)
{
  L.big_pairs = 0;
  L.big_delta = L.big_tmin = 0.f;
  for (int k = 0; k < 8; k++)
    L.big_qmin[k] = std::numeric_limits<float>::infinity();
#ifdef PT_DEV_KERNELS
  static const bool off = [] {
    const char *e = getenv("RT_HIP_NO_BIG_PRUNE"); /* development switch (A/B) */
    return e && e[0] == '1';
  }();
#else
  const bool off = false;
#endif
  /* the kernels whose sphere filter is the sign-test form from LDS: sphere-only small scenes, and hierarchy scenes whose
   * spheres fit the staging (the parked-walk kernels filter the spheres alone) */
  const bool sign_form = !scene->view.wide_range &&
                         (pt_geom_in_lds(scene->view) ? (scene->view.n_triangles == 0 ? pt_filter_in_lds(scene->view) : !pt_filter_in_lds(scene->view))
                                                      : (scene->view.n_triangles == 0)); /* pt_render_tiles_pool_mem_s, pt_render_tiles_refr_pool_mem
                                                                             * (scenes it takes by preference, pt_prefer_streaming, satisfy the first arm) */
  if (off || scene->n_big < 2 || !sign_form)
    return;
  const double e = 5.9604644775390625e-08, f = 1.0 / 16.0;
  double delta = 0, tmin = 0;
  for (int k = 0; k < scene->n_big; k++)
  {
    const double r = scene->big_r[k], c = scene->big_c[k], A = c + near_R + filt_shift;
    const double g = std::fabs(c * c - r * r);
    /* W >= r2_hi' - r^2 of the table: pt_build_filter widens by pt_sign_widen_total(A_table, g) with A_table = |c| + near_R <= A
     * (the function is increasing in A), then rounds kq DOWN to fp32 (at most 2 e |kq| more: inside the factor 1.001) */
    const double W = pt_sign_widen_total(A, g) * 1.001, E = 28.0 * e * A * A + 6.0 * e * g;
    const double qmin = f * f * r * r + W + E;
    const double bias = (W + E) / (2.0 * f * r);
    if (!(qmin < 1e30) || !(bias < 1e3))
      return;
    L.big_qmin[k] = (float)(qmin * (1.0 + 4.0 * e));
    delta = std::fmax(delta, 1.5 * (22.4 * e * A + bias));
    tmin = std::fmax(tmin, 2.0 * (filt_shift * 1.0001 + 11.2 * e * A));
  }
  L.big_delta = (float)(delta * (1.0 + 4.0 * e));
  L.big_tmin = (float)(tmin * (1.0 + 4.0 * e));
  L.big_pairs = (uint32_t)scene->n_big / 2u;
}

/* How far on the outer side of a hull facet F (pt_build_hull_flags) a ray must point, mu < m . d, to be certain
 * not to meet a triangle.  With u = 2^-53, sigma = |e1||e2| / |e1 x e2| <= 16 (the flag's shape limit), D >= |o - v0|
 * and the hit distance (3 (near_R + extent) covers both):
 *   - the computed hit point on F lies within delta of F's plane: N . (o + t d - v0) = e2 . q - t a exactly (N = e1 x e2,
 *     q = s x e1, a = e1 . (d x e2): intersect_triangle's own quantities), which vanishes for the exact t; the computed
 *     t carries 6 u (|s| + t) |e1||e2| / |N| + 3 u |s| of plane distance, the point's own three roundings 6 u D more:
 *     delta <= 26 u sigma D <= 1.4e-13 (near_R + extent);
 *   - every triangle point p has m . (p - v0) <= tau = 2^-43 extent;
 *   - so a hit needs t <= (tau + delta) / mu, and mu = 4 (tau + delta) / EPSILON puts that at EPSILON / 4, where the
 *     exact test (t > EPSILON, raytracer.c:150) rejects it, its own rounding of t (relative ~1e-12) included.
 * Never below 1e-3; scenes so large that mu reaches 1 simply never skip a walk.  D holds for rays whose hit
 * distance is at most 2 near_R: then |o - v0| <= 1.0001 x that + the facet's size as well; trace_step drops the
 * facet's mark for any other (a bounce that came in from a far point of a wall-sized sphere, say). */
double hull_margin_for(const RtHipScene *scene, double near_R)
{
  if (!scene->hull_flags || !(near_R < 1e150))
    return 2.0; /* no ray has m . d > 2 */
  const double extent = scene->mesh_c_norm + scene->mesh_R;
  const double tau = 1.1368683772161603e-13 * extent, delta = 1.4e-13 * (near_R + extent);
  return std::fmax(1e-3, 4.0 * (tau + delta) / 1e-8);
}

/* What a launch of rt_hip_render_tiles_chunked and an accumulation (rt_hip_accum_create) have in common before the plan: the
 * parameters checked, and the launch's scene- and camera-dependent fields.  *empty: no tile to render (not an error). */
int launch_prepare(const RtHipScene *scene, const RtHipCamera *camera, const RtHipParams *params, PtLaunch &L, bool *empty)
{
  const int rc = check_params(params);
  if (rc)
    return rc;
  const bool cast_ray = params->integrator == RT_HIP_CAST_RAY;
  if (!cast_ray && scene->view.any_refract && params->max_depth > PT_REFRACT_MAX_DEPTH)
    return fail(RT_HIP_ELIMIT, "scenes with M_REFRACTION materials support max_depth <= %d (two rays per "
                               "refractive hit, raytracer.c:523-529; the pending-ray stack is fixed)",
                PT_REFRACT_MAX_DEPTH);
  if (cast_ray && scene->any_mirror_glass && params->max_depth > PT_REFRACT_MAX_DEPTH)
    return fail(RT_HIP_ELIMIT, "cast_ray with M_REFLECTION|M_REFRACTION materials supports max_depth <= %d (two "
                               "rays per such hit, raytracer.c:609-628; the pending-ray stack is fixed)",
                PT_REFRACT_MAX_DEPTH);
  const uint32_t tx = tiles_x_of(params->width), ty = tiles_y_of(params->height);
  const uint64_t n_tiles = (uint64_t)tx * ty;
  *empty = params->tile_count == 0;
  if (*empty)
    return RT_HIP_OK;
  if (params->tile_stride == 0 && params->tile_count > 1)
    return fail(RT_HIP_EINVAL, "tile_stride must be >= 1");
  const uint64_t last = (uint64_t)params->tile_first + (uint64_t)(params->tile_count - 1) * params->tile_stride;
  if (last >= n_tiles)
    return fail(RT_HIP_EINVAL, "tile range [%u + k*%u, k < %u] exceeds the image's %llu tiles", params->tile_first,
                params->tile_stride, params->tile_count, (unsigned long long)n_tiles);

  memset(&L, 0, sizeof L);
  L.scene = scene->view;
  memcpy(L.cam.pos, camera->position, sizeof L.cam.pos);
  memcpy(L.cam.horizontal, camera->horizontal, sizeof L.cam.horizontal);
  memcpy(L.cam.vertical, camera->vertical, sizeof L.cam.vertical);
  memcpy(L.cam.llc, camera->lower_left_corner, sizeof L.cam.llc);
  L.width = params->width;
  L.height = params->height;
  L.samples = params->samples;
  L.max_depth = params->max_depth;
  L.seed = params->seed;
  {
    /* Ray origins are the camera or points on primitives.  The packed-fp32 filter of
     * scan_filtered is built for origins within near_R; a ray starting farther out (e.g. on
     * the far side of a radius-1e4 "wall" sphere) is still traced exactly, it just skips
     * the filter.  near_R only trades filter tightness against that fallback. */
    const double *c = camera->position;
    const double cam = std::sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
    L.near_R = 1.5 * (cam + scene->reach) + 1.0;
    if (!(L.near_R < RT_NEAR_R_LIMIT))
      return fail(RT_HIP_EINVAL, "scene extent %g is not a usable finite bound", L.near_R);
    L.near_R2 = L.near_R * L.near_R;
    L.filt_shift = 12.0 * 5.9604644775390625e-08 * (scene->max_center + L.near_R) * (1.0 + 1e-9);
    mesh_bound_for(scene, L.near_R, L.mesh_bound);
    big_prune_for(scene, L.near_R, L.filt_shift, L);
    L.hull_margin = hull_margin_for(scene, L.near_R);
#ifdef PT_DIAG
    { /* the diagnostic build only: walk the rays the probe or the hull rule would not walk, and count any that find a triangle */
      const char *flag = getenv("RT_HIP_DIAG_WALK_REJECTED");
      L.diag_flags = (flag && flag[0] == '1') ? 1u : 0u;
      /* RT_HIP_DIAG_PARK_COUNTS=1: the caller's counters hold 64 words, not 48: the retry stack's five go to stats[4 + 44] .. [4 + 48] */
      const char *park = getenv("RT_HIP_DIAG_PARK_COUNTS");
      L.diag_flags |= (park && park[0] == '1') ? 2u : 0u;
    }
#endif
#ifdef PT_PHASE
    { /* the phase build only (tools/grid_tail.py): RT_HIP_PHASE_WG_TIMES=1: the caller's counters hold 80 + 2 x workgroups words */
      const char *times = getenv("RT_HIP_PHASE_WG_TIMES");
      L.diag_flags |= (times && times[0] == '1') ? 4u : 0u;
    }
#endif
    L.background = 10 / 255.0;
    L.t_start = 1.7976931348623157e308; /* DBL_MAX */
    L.w_minus_1 = (double)params->width - 1.0;
    L.h_minus_1 = (double)params->height - 1.0;
    L.inv_w_minus_1 = 1.0 / L.w_minus_1; /* IEEE division on the host: correctly rounded */
    L.inv_h_minus_1 = 1.0 / L.h_minus_1;
  }
  {
    /* Fixed-point scale of the per-pixel sums (pt_render_tiles): a sample's radiance is
     * sum_k T_k (.) e_k with throughput T <= 1 (albedo/prob <= 1, cos <= 1) over at most
     * max_depth + 2 events -- pt_acc_scale_exp (pt_device.h), which pt_classify reads too: whether these sums are
     * fine enough for the launch (pt_fixed_sums_fit) picks the kernel. */
    const int s = pt_acc_scale_exp(scene->max_emission, params->samples, params->max_depth);
    if (s == INT32_MIN)
      return fail(RT_HIP_EINVAL, "emission magnitudes give no finite radiance bound (%g)", scene->max_emission);
    L.acc_scale = std::ldexp(1.0, s);
    L.acc_inv_scale = std::ldexp(1.0, -s);
  }
  L.tile_first = params->tile_first;
  L.tile_stride = params->tile_stride;
  L.tile_count = params->tile_count;
  L.tiles_x = tx;
  L.integrator = cast_ray ? 1u : 0u;
  return RT_HIP_OK;
}

/* ... and, with the scene's device current: the device's status word and the parked-walk workspace */
int launch_device_state(const RtHipScene *scene, PtLaunch &L)
{
  const bool cast_ray = L.integrator == 1u;
  const int rc = status_word_for(scene->device, &L.status);
  if (rc)
    return rc;
  if (scene->view.n_bvh_nodes != 0 && !cast_ray)
  {
    /* parked-walk workspace: the device's shared pool (flags + rings).  Without it the pick table's park = NO rows apply
     * (the lane-waiting kernels), and rt_hip_kernel_name reports those. */
    std::lock_guard<std::mutex> lock(scene->table_mutex);
    if (!scene->park_tried)
    {
      scene->park_tried = true;
      scene->park_ws = park_acquire_ws(scene->device, &scene->park_slots_per_xcd);
    }
    if (scene->park_ws)
    {
      L.park_flags = reinterpret_cast<uint32_t *>(scene->park_ws);
      L.park_ws = scene->park_ws + park_flag_bytes(scene->park_slots_per_xcd);
      L.park_slots_per_xcd = scene->park_slots_per_xcd;
    }
  }
  return RT_HIP_OK;
}

/* What a launch of `scene` asks the plan (pt_kernel.hip, pt_plan_launch).  wide_pend_ok starts out true: who knows that the wide
 * pending-ray pool cannot be had says so afterwards. */
PtPlanAsk ask_for(const RtHipScene *scene, uint32_t integrator, int32_t samples, int32_t max_depth, uint32_t sample_chunks,
                  bool have_chunk_ws, uint32_t tile_count, bool have_park_ws)
{
  return {.integrator = integrator, .samples = samples, .max_depth = max_depth, .max_emission = scene->max_emission,
          .sample_chunks = sample_chunks, .have_chunk_ws = have_chunk_ws, .tile_count = tile_count, .have_park_ws = have_park_ws,
          .wide_pend_ok = true};
}

/* Which kernel, how many sample chunks it runs, which pools it needs: the plan of the prepared launch L, and the pending-ray pool
 * it asks for, taken through take_pool(entries, columns, L).  The parked-walk refraction kernels want four times the stacks per
 * slot (1.2 GB at depth 5, 5.7 GB at 32): where that cannot be had, the pool of the other kernels will do -- planned again, the
 * table's fit = NO row names the static kernel of the family.  Sets L.sample_chunks and L.acc_windows. */
template <class PoolFn>
int plan_launch(const RtHipScene *scene, PtLaunch &L, uint32_t sample_chunks, bool have_chunk_ws, PoolFn take_pool, PtPlan *out)
{
  PtPlanAsk ask = ask_for(scene, L.integrator, L.samples, L.max_depth, sample_chunks, have_chunk_ws, L.tile_count, L.park_ws != nullptr);
  PtPlan plan = pt_plan_launch(L.scene, ask);
  int rc = plan.pend_entries ? take_pool(plan.pend_entries, plan.pend_columns, L) : RT_HIP_OK;
  if (rc == RT_HIP_ENOMEM && plan.pend_columns > PT_PEND_COLUMNS)
  {
    ask.wide_pend_ok = false;
    plan = pt_plan_launch(L.scene, ask);
    rc = plan.pend_entries ? take_pool(plan.pend_entries, plan.pend_columns, L) : RT_HIP_OK;
  }
  L.sample_chunks = plan.sample_chunks;
  L.acc_windows = plan.windowed ? 1u : 0u;
  *out = plan;
  return rc;
}

void accum_free(RtHipAccum *a)
{
  if (!a)
    return;
  DeviceScope scope(a->scene->device);
  (void)hipDeviceSynchronize(); /* no pass may still be using what it owns */
  a->scene->live_accums--;
  delete a;
}

/* the freeze state of an accumulation, made at its first freeze: every slot live */
int accum_adapt_state(RtHipAccum *a)
{
  if (a->tile_samples)
    return RT_HIP_OK;
  const size_t n = a->L.tile_count;
  const size_t bytes = (2 * n + 1) * sizeof(uint32_t) + n;
  DeviceBuffer buf;
  const hipError_t e = buf.alloc(bytes);
  if (e != hipSuccess)
    return fail(RT_HIP_ENOMEM, "freeze state (%zu KB): %s", bytes >> 10, hipGetErrorString(e));
  HIP_TRY(hipMemset(buf.ptr, 0, bytes));
  HIP_TRY(hipStreamSynchronize(nullptr));
  a->tile_samples = std::move(buf);
  a->slot_list = a->tile_samples.at<uint32_t>() + n;
  a->d_live_count = a->slot_list + n;
  a->keep = reinterpret_cast<uint8_t *>(a->d_live_count + 1);
  a->live_count = (uint32_t)n;
  return RT_HIP_OK;
}

int accum_freeze(RtHipAccum *a, const float *d_error, const uint8_t *h_keep, double threshold, uint32_t dilate, uint32_t *live_count,
                        void *stream)
{
  if (live_count)
    *live_count = 0;
  if (!a)
    return fail(RT_HIP_EINVAL, "accumulation is NULL");
  if (!d_error && !h_keep)
    return fail(RT_HIP_EINVAL, "a freeze needs the tile errors or a keep mask");
  if (dilate > 2u)
    return fail(RT_HIP_EINVAL, "dilate is 0 .. 2 tiles, not %u", dilate);
  if (a->done < 1)
    return fail(RT_HIP_EINVAL, "the accumulation holds no sample yet");
  if (a->broken)
    return fail(RT_HIP_ERUNTIME, "the accumulation is unusable: an earlier freeze failed on the device");
  const PtLaunch &L = a->L;
  if (d_error && !(threshold > 0.0))
  { /* a threshold <= 0 (or NaN) freezes nothing: the frame stays the uniform one */
    if (live_count)
      *live_count = a->tile_samples ? a->live_count : L.tile_count;
    return RT_HIP_OK;
  }
  DeviceScope scope(a->scene->device);
  HIP_TRY(scope.status);
  int rc = accum_adapt_state(a);
  if (rc)
    return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipError_t e = hipSuccess;
  if (!d_error)
    e = hipMemcpyAsync(a->keep, h_keep, L.tile_count, hipMemcpyHostToDevice, st);
  if (e == hipSuccess)
    e = pt_launch_tile_freeze(d_error, threshold, (int)dilate, a->keep, a->tile_samples.at<uint32_t>(), L.width, L.height, L.tile_first, L.tile_stride,
                              L.tile_count, (uint32_t)a->done, a->slot_list, a->d_live_count, st);
  uint32_t n = 0;
  if (e == hipSuccess)
    e = hipMemcpyAsync(&n, a->d_live_count, sizeof n, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess)
    e = hipStreamSynchronize(st); /* the next pass's grid needs the count on the host */
  if (e != hipSuccess)
  { /* the device may have rewritten the counts and the list: the host's copy of the live count cannot be trusted any more */
    a->broken = true;
    return fail(RT_HIP_ERUNTIME, "freeze: %s", hipGetErrorString(e));
  }
  a->live_count = n;
  a->any_frozen = a->any_frozen || n < L.tile_count;
  if (live_count)
    *live_count = n;
  return RT_HIP_OK;
}

/* the passes and checkpoints of rt_hip_accum_run_adaptive.  *seconds grows by every timed piece that ran, also when a later one
 * fails or the caller cancels. */
int adaptive_passes(RtHipAccum *a, const RtHipAdaptParams *p, uint64_t *h_stats,
                    int (*on_checkpoint)(void *user, int32_t samples_done, uint32_t live_tiles), void *user, double *seconds)
{
  const PtLaunch &L = a->L;
  const size_t tile_vals = (size_t)L.tile_count * PT_TILE_PIXELS * 3;
  const bool estimate = p->threshold > 0.0;
  if (estimate && !a->adapt_buf)
  {
    const hipError_t e = a->adapt_buf.alloc((2 * tile_vals + L.tile_count) * sizeof(float));
    if (e != hipSuccess)
      return fail(RT_HIP_ENOMEM, "adaptive buffers: %s", hipGetErrorString(e));
  }
  float *prev = a->adapt_buf.at<float>(), *cur = prev + tile_vals, *err = prev + 2 * tile_vals;
  int32_t targets[32];
  const int n_targets = rt_hip_adapt_schedule(a->budget, p->min_samples, targets, 32);
  EventPair timer;
  HIP_TRY(timer.create());
  for (int i = 0; i < n_targets; i++)
  {
    if (targets[i] > a->done)
    {
      double pass_seconds = 0;
      const int rc = rt_hip_accum_add_host(a, targets[i] - a->done, h_stats, &pass_seconds);
      *seconds += pass_seconds;
      if (rc)
        return rc;
    }
    if (targets[i] == a->budget)
      break; /* the last pass is followed by no estimate */
    uint32_t live = rt_hip_accum_live_tiles(a);
    if (estimate)
    { /* (a threshold <= 0 freezes nothing: no resolve, no estimate, the passes alone) */
      HIP_TRY(timer.start(nullptr));
      int rc = rt_hip_accum_resolve(a, i == 0 ? prev : cur, nullptr, nullptr);
      if (i > 0 && !rc)
      {
        /* (every slot is estimated, the frozen ones too: both resolves divide a frozen slot's unchanged sums by its own count, so
         * cur == prev there, its error is +0.0 and it never votes in the dilation) */
        rc = rt_hip_tile_error(cur, prev, L.width, L.height, L.tile_first, L.tile_stride, L.tile_count, err, nullptr);
        if (!rc)
          rc = rt_hip_accum_freeze(a, err, p->threshold, p->dilate, &live, nullptr);
        std::swap(prev, cur);
      }
      if (rc)
        return rc;
      HIP_TRY(timer.stop(nullptr));
      HIP_TRY(timer.wait());
      float ms = 0.f;
      HIP_TRY(timer.elapsed_ms(&ms));
      *seconds += 1e-3 * (double)ms; /* the checkpoint's own timer, added to the passes' (rt_hip_accum_add_host) */
    }
    if (i > 0 && on_checkpoint && on_checkpoint(user, a->done, live))
      return fail(RT_HIP_ECANCELLED, "adaptive render cancelled at %d samples", a->done);
    if (i > 0 && live == 0u)
      break;
  }
  return RT_HIP_OK;
}

bool aov_any(const RtHipAov *a) { return a && (a->albedo || a->normal || a->depth || a->object || a->hits); }

/* ---- rt_hip_render_image: the whole image on n_devices GPUs of this process ------------------------------------------------
 * Device g renders tiles g, g+G, g+2G, ... into its own compact buffer; the buffers are gathered on
 * device 0 with grouped ncclSend/ncclRecv (point-to-point over xGMI: a gather
 * to one root uses the root's 7 direct links concurrently, there is no ring),
 * scattered to the row-major image there, and copied to the host.
 *
 * Everything rt_hip_render_image() needs between calls -- per device: the uploaded scene, a
 * stream, timing events, the compact tile buffers, counters, the chunk workspace; on device 0 the
 * gathered tiles and the row-major images; and the RCCL communicators -- is kept in one cached
 * context and reused while the device count, the image size and the scene's bytes stay the same
 * (an animation loop calling render() per frame re-creates nothing; ncclCommInitAll alone costs
 * tens of milliseconds per call at 8 devices).  rt_hip_release_cache() drops it. */
constexpr size_t TILE_VALS = (size_t)PT_TILE_PIXELS * 3; /* floats -- or bytes -- of a tile */

struct ImageCtx
{
  struct Dev
  {
    RtHipScene *scene = nullptr;
    hipStream_t stream = nullptr;
    EventPair timer;           /* around the device's share */
    hipEvent_t done = nullptr; /* its tiles are complete (what a same-device copy or the lead's sends wait for) */
    DeviceBuffer tiles, tiles8, stats, ws;
    uint32_t count = 0;    /* tiles of its share */
    size_t first_slot = 0; /* where its segment begins in the gathered tiles */
  };
  int G = 0, W = 0, H = 0;
  /* logical device g runs on physical device phys[g] (rt_hip_set_device_map; the identity without a map).  Logical devices
   * that share a physical one each keep their own scene, stream and tile buffers -- everything above the gather is the same
   * code as with G distinct GPUs.  comm_of[g]: index of phys[g] among the DISTINCT physical devices = its RCCL rank (RCCL
   * refuses two ranks on one device); lead[g]: the first logical device on phys[g], whose stream carries that rank's sends. */
  std::vector<int> phys, comm_of, lead;
  int n_phys = 0;
  bool force_comm = false; /* RT_HIP_FORCE_COMM=1: communicators and the gather's send/recv block even with one device */
  std::vector<unsigned char> scene_bytes; /* the scene this context was built for (scene_walk's runs): compared run by run */
  std::vector<Dev> dev;
  std::vector<ncclComm_t> comms; /* one per distinct physical device (comm_of) */
  DeviceBuffer all_tiles, all_tiles8, image, image8; /* on the root, phys[0] */
  uint64_t builds = 0; /* how many times a context was (re)built: exposed for tests */
  uint64_t updates = 0; /* how many times its scenes' vertices were moved in place instead (rt_hip_set_scene_updates) */
  uint64_t rebuilds = 0; /* in how many of those frames a scene's hierarchy was rebuilt in place (rt_hip_set_bvh_rebuild_ratio) */
  int bvh_builder = RT_HIP_BVH_HOST; /* who built the scenes' hierarchies (rt_hip_set_bvh_builder) */
};
/* (never destroyed: at process exit the members' destructors would call into a HIP runtime that may be gone already) */
ImageCtx &g_ctx = *new ImageCtx;
std::mutex g_ctx_mutex;
double g_last_phases[3] = {0, 0, 0}; /* rt_hip_last_image_phases */

/* The logical -> physical device map of rt_hip_render_image (rt_hip_set_device_map, or RT_HIP_DEVICE_MAP=0,0,1 read at
 * the first frame).  Empty = the identity.  Guarded by g_ctx_mutex. */
std::vector<int> g_device_map;
bool g_device_map_env_read = false;
int g_bvh_builder = RT_HIP_BVH_HOST; /* rt_hip_set_bvh_builder: the builder of the cached scenes.  Guarded by g_ctx_mutex. */
bool g_scene_updates = false; /* rt_hip_set_scene_updates: moved vertices update the cached scenes in place.  Guarded by g_ctx_mutex. */
bool g_material_updates = false; /* rt_hip_set_material_updates: changed flags, colours and emission update the cached scenes in place.  Guarded by g_ctx_mutex. */
double g_bvh_rebuild_ratio = 0; /* rt_hip_set_bvh_rebuild_ratio: 0 = never; else rt_hip_scene_maintain_bvh's max_ratio after such an update.  Guarded by g_ctx_mutex. */

void device_map_from_env()
{
  if (g_device_map_env_read)
    return;
  g_device_map_env_read = true;
  const char *e = getenv("RT_HIP_DEVICE_MAP");
  if (!e || !*e || !g_device_map.empty())
    return;
  std::vector<int> m;
  for (const char *p = e; *p;)
  {
    char *end = nullptr;
    const long v = strtol(p, &end, 10);
    if (end == p || v < 0 || v > 63)
      return; /* malformed: ignored as a whole */
    m.push_back((int)v);
    p = end;
    if (*p == ',')
      p++;
    else if (*p)
      return;
  }
  g_device_map = m;
}

/* What needs an order: the streams drained, then the communicators, then each device's members with that device current.
 * `builds`, `updates` and `rebuilds` survive. */
void ctx_release(ImageCtx &c)
{
  int prev = 0;
  (void)hipGetDevice(&prev);
  for (int g = 0; g < (int)c.dev.size(); g++)
    if (c.dev[g].stream)
    {
      (void)hipSetDevice(c.phys[g]);
      (void)hipStreamSynchronize(c.dev[g].stream);
    }
  for (int r = 0; r < (int)c.comms.size(); r++)
    if (c.comms[r])
    {
      for (int g = 0; g < (int)c.comm_of.size(); g++)
        if (c.comm_of[g] == r)
        {
          (void)hipSetDevice(c.phys[g]);
          break;
        }
      (void)ncclCommDestroy(c.comms[r]);
    }
  for (int g = 0; g < (int)c.dev.size(); g++)
  {
    (void)hipSetDevice(c.phys[g]);
    ImageCtx::Dev &d = c.dev[g];
    if (d.done) (void)hipEventDestroy(d.done);
    if (d.stream) (void)hipStreamDestroy(d.stream);
    rt_hip_scene_destroy(d.scene);
    d = ImageCtx::Dev(); /* its timer and buffers */
  }
  if (!c.phys.empty())
    (void)hipSetDevice(c.phys[0]);
  const uint64_t builds = c.builds, updates = c.updates, rebuilds = c.rebuilds;
  c = ImageCtx(); /* the root's gathered tiles and images */
  c.builds = builds;
  c.updates = updates;
  c.rebuilds = rebuilds;
  (void)hipSetDevice(prev);
}

/* The error exit of the image context, made once g_ctx_mutex is held: unless keep() was called, leaving the scope drops the cached
 * context -- a failure leaves it in an unknown state.  The caller's device is put back either way. */
struct CtxGuard
{
  int prev = 0;
  bool kept = false;
  CtxGuard() { (void)hipGetDevice(&prev); }
  CtxGuard(const CtxGuard &) = delete;
  void keep() { kept = true; }
  ~CtxGuard()
  {
    if (!kept)
      ctx_release(g_ctx);
    (void)hipSetDevice(prev);
  }
};

/* Everything that defines the scene, field by field (struct padding is not part of the scene), as runs of bytes handed
 * to `f(ptr, n, kind)` in a fixed order (kind: RUN_VERTICES, the run is a mesh's RtHipVertex array; RUN_SPHERE, a sphere's ten doubles, radius and centre first, colour and emission behind them; RUN_FLAGS, an object's flags; RUN_MATERIAL, a mesh's colour and emission; RUN_OTHER).  The cached context keeps the concatenation (ImageCtx::scene_bytes) and is reused only
 * while a call's scene equals it byte for byte: scene_matches() compares run by run (memcmp, stopping at the first
 * difference) against the kept copy -- no per-call serialisation, no hashing: a frame of config 5's mesh used to rebuild
 * and hash 1.2 MB on the host inside every rt_hip_render_image() call (round-3 advisor finding). */
enum { RUN_OTHER = 0, RUN_VERTICES = 1, RUN_SPHERE = 2, RUN_FLAGS = 3, RUN_MATERIAL = 4 };
template <class F>
void scene_walk(const RtHipSphere *spheres, size_t n_spheres, const RtHipMesh *meshes, size_t n_meshes, F &&f)
{
  f(&n_spheres, sizeof n_spheres, RUN_OTHER);
  f(&n_meshes, sizeof n_meshes, RUN_OTHER);
  for (size_t i = 0; i < n_spheres; i++)
  {
    f(&spheres[i].flags, sizeof spheres[i].flags, RUN_FLAGS);
    f(&spheres[i].radius, sizeof(double) * 10, RUN_SPHERE); /* radius, center, color, emission are contiguous doubles */
  }
  for (size_t m = 0; m < n_meshes; m++)
  {
    f(&meshes[m].flags, sizeof meshes[m].flags, RUN_FLAGS);
    f(meshes[m].color, sizeof(double) * 6, RUN_MATERIAL); /* color, emission */
    f(&meshes[m].num_triangles, sizeof meshes[m].num_triangles, RUN_OTHER);
    if (meshes[m].vertices)
      f(meshes[m].vertices, meshes[m].num_triangles * 3 * sizeof(RtHipVertex), RUN_VERTICES);
  }
}

/* SCENE_MOVED: equal but for vertex positions (MOVED_VERTICES), sphere centres and radii (MOVED_SPHERES) and flags, colours and
 * emission (MOVED_MATERIALS), as *moved says: what an update in place can take, each kind where its switch allows it */
enum SceneMatch { SCENE_DIFFERS = 0, SCENE_SAME = 1, SCENE_MOVED = 2 };
enum { MOVED_VERTICES = 1, MOVED_SPHERES = 2, MOVED_MATERIALS = 4 };

SceneMatch scene_matches(const std::vector<unsigned char> &kept, const RtHipSphere *spheres, size_t n_spheres,
                         const RtHipMesh *meshes, size_t n_meshes, int *moved_what)
{
  size_t at = 0;
  bool same = true;
  int moved = 0;
  scene_walk(spheres, n_spheres, meshes, n_meshes, [&](const void *p, size_t n, int kind) {
    if (!same)
      return;
    if (n > kept.size() - at)
      same = false;
    else if (memcmp(kept.data() + at, p, n) != 0)
    {
      /* a vertex run may differ in positions; the tex coordinates behind each position must not */
      const unsigned char *a = kept.data() + at, *b = static_cast<const unsigned char *>(p);
      const size_t tex = offsetof(RtHipVertex, tex);
      same = kind != RUN_OTHER;
      if (kind == RUN_VERTICES)
      {
        for (size_t v = 0; same && v < n / sizeof(RtHipVertex); v++)
          same = memcmp(a + v * sizeof(RtHipVertex) + tex, b + v * sizeof(RtHipVertex) + tex, sizeof(RtHipVertex) - tex) == 0;
        moved |= MOVED_VERTICES;
      }
      else if (kind == RUN_SPHERE)
      { /* the radius and the centre are the sphere's place; the colour and the emission behind them its material */
        if (memcmp(a, b, 4 * sizeof(double)) != 0)
          moved |= MOVED_SPHERES;
        if (memcmp(a + 4 * sizeof(double), b + 4 * sizeof(double), n - 4 * sizeof(double)) != 0)
          moved |= MOVED_MATERIALS;
      }
      else
        moved |= MOVED_MATERIALS;
    }
    at += n;
  });
  if (!same || at != kept.size())
    return SCENE_DIFFERS;
  *moved_what = moved;
  return moved ? SCENE_MOVED : SCENE_SAME;
}

void scene_serialise(std::vector<unsigned char> &bytes, const RtHipSphere *spheres, size_t n_spheres, const RtHipMesh *meshes,
                     size_t n_meshes)
{
  bytes.clear();
  scene_walk(spheres, n_spheres, meshes, n_meshes, [&](const void *p, size_t n, int) {
    const unsigned char *b = static_cast<const unsigned char *>(p);
    bytes.insert(bytes.end(), b, b + n);
  });
}

/* makes g_ctx fit this call (device count and map, image size, scene); caller holds g_ctx_mutex and a CtxGuard */
int ctx_prepare(const RtHipSphere *spheres, size_t n_spheres, const RtHipMesh *meshes, size_t n_meshes, int G,
                const std::vector<int> &phys, int W, int H)
{
  /* RT_HIP_FORCE_COMM=1: build the RCCL communicator(s) and run the gather's grouped send / recv block even where no
   * tile has to change devices (one device, or logical devices that all share one): every segment then travels through
   * RCCL as a send to self -- how a one-GPU box exercises library load, bootstrap, communicator creation / destruction
   * and the send / recv kernels of the N > 1 path */
  const char *fc = getenv("RT_HIP_FORCE_COMM");
  const bool force_comm = fc && fc[0] == '1';
  ImageCtx &c = g_ctx;
  if (c.G == G && c.W == W && c.H == H && c.force_comm == force_comm && (int)c.dev.size() == G && c.phys == phys &&
      c.bvh_builder == g_bvh_builder)
  {
    int moved = 0;
    const SceneMatch match = scene_matches(c.scene_bytes, spheres, n_spheres, meshes, n_meshes, &moved);
    if (match == SCENE_SAME)
      return RT_HIP_OK;
    const bool may_move = !(moved & (MOVED_VERTICES | MOVED_SPHERES)) || g_scene_updates;
    const bool may_recolour = !(moved & MOVED_MATERIALS) || g_material_updates;
    if (match == SCENE_MOVED && may_move && may_recolour)
    { /* only vertex positions, sphere centres and radii differ (rt_hip_set_scene_updates), or flags, colours and emission
       * (rt_hip_set_material_updates): every device's scene takes them in place, by the update of each kind that differs; a
       * failure drops the context (CtxGuard) */
      if (moved & MOVED_VERTICES)
      {
        size_t n_tri = 0;
        for (size_t m = 0; m < n_meshes; m++)
          n_tri += meshes[m].num_triangles;
        std::vector<double> pos(9 * n_tri);
        size_t at = 0;
        for (size_t m = 0; m < n_meshes; m++)
          for (size_t k = 0; k < 3 * meshes[m].num_triangles; k++, at += 3)
            memcpy(&pos[at], meshes[m].vertices[k].pos, 3 * sizeof(double));
        for (int g = 0; g < G; g++)
        {
          const int rc = rt_hip_scene_update_vertices_host(c.dev[g].scene, pos.data(), n_tri);
          if (rc)
            return rc;
        }
        if (g_bvh_rebuild_ratio != 0)
        { /* the refitted trees priced against the trees as built; rebuilt in place where the ratio is above the setting */
          bool any = false;
          for (int g = 0; g < G; g++)
          {
            int rebuilt = 0;
            const int rc = rt_hip_scene_maintain_bvh(c.dev[g].scene, g_bvh_rebuild_ratio, nullptr, &rebuilt);
            if (rc)
              return rc;
            any = any || rebuilt != 0;
          }
          if (any)
            c.rebuilds++;
        }
      }
      if (moved & MOVED_SPHERES)
      {
        std::vector<double> sph(SCENE_SPHERE_IN * n_spheres);
        for (size_t i = 0; i < n_spheres; i++)
        {
          memcpy(&sph[SCENE_SPHERE_IN * i], spheres[i].center, 3 * sizeof(double));
          sph[SCENE_SPHERE_IN * i + 3] = spheres[i].radius;
        }
        for (int g = 0; g < G; g++)
        {
          const int rc = rt_hip_scene_update_spheres_host(c.dev[g].scene, sph.data(), n_spheres);
          if (rc)
            return rc;
        }
      }
      if (moved & MOVED_MATERIALS)
      {
        const size_t n_mat = n_spheres + n_meshes;
        std::vector<double> mat(SCENE_MATERIAL_IN * n_mat);
        std::vector<uint32_t> flags(n_mat);
        for (size_t i = 0; i < n_mat; i++)
        {
          const bool sph = i < n_spheres;
          memcpy(&mat[SCENE_MATERIAL_IN * i], sph ? spheres[i].color : meshes[i - n_spheres].color, 3 * sizeof(double));
          memcpy(&mat[SCENE_MATERIAL_IN * i + 3], sph ? spheres[i].emission : meshes[i - n_spheres].emission, 3 * sizeof(double));
          flags[i] = sph ? spheres[i].flags : meshes[i - n_spheres].flags;
        }
        for (int g = 0; g < G; g++)
        {
          const int rc = rt_hip_scene_update_materials_host(c.dev[g].scene, mat.data(), flags.data(), n_mat);
          if (rc)
            return rc;
          /* the chunk workspace was sized for the scene's flag class as it was (rt_hip_scene_chunk_workspace_bytes: the windowed
           * sums of the M_REFRACTION forms are six times the plain record): the next chunked launch sizes it anew, as a rebuilt
           * context would.  The frames are synchronous and the update has drained the scene: nothing reads it any more. */
          HIP_TRY(hipSetDevice(c.phys[g]));
          c.dev[g].ws.release();
        }
      }
      scene_serialise(c.scene_bytes, spheres, n_spheres, meshes, n_meshes);
      c.updates++;
      return RT_HIP_OK;
    }
  }
  ctx_release(c);
  c.builds++;
  c.dev.resize(G);
  c.phys = phys;
  c.comm_of.assign(G, 0);
  c.lead.assign(G, 0);
  c.n_phys = 0;
  for (int g = 0; g < G; g++)
  {
    int first = g;
    for (int j = 0; j < g; j++)
      if (phys[j] == phys[g])
      {
        first = j;
        break;
      }
    c.lead[g] = first;
    c.comm_of[g] = first == g ? c.n_phys++ : c.comm_of[first];
  }
  c.comms.assign(c.n_phys, nullptr);
  const uint32_t n_tiles = tiles_x_of(W) * tiles_y_of(H);
  const size_t n_px = (size_t)W * H;
  size_t first_slot = 0;
  for (int g = 0; g < G; g++)
  {
    ImageCtx::Dev &d = c.dev[g];
    d.count = (n_tiles > (uint32_t)g) ? (n_tiles - g + G - 1) / G : 0;
    d.first_slot = first_slot;
    first_slot += d.count;
    RtHipSceneOptions opts;
    rt_hip_scene_options_defaults(&opts);
    opts.bvh_builder = (uint32_t)g_bvh_builder;
    const int rc = rt_hip_scene_create_opts(spheres, n_spheres, meshes, n_meshes, phys[g], &opts, &d.scene);
    if (rc)
      return rc;
    HIP_TRY(hipSetDevice(phys[g]));
    HIP_TRY(hipStreamCreate(&d.stream));
    HIP_TRY(d.timer.create());
    HIP_TRY(hipEventCreateWithFlags(&d.done, hipEventDisableTiming));
    const size_t slots = d.count ? d.count : 1;
    HIP_TRY(d.tiles.alloc(slots * TILE_VALS * sizeof(float)));
    HIP_TRY(d.tiles8.alloc(slots * TILE_VALS));
    HIP_TRY(d.stats.alloc(RT_HIP_NSTATS * sizeof(uint64_t)));
  }
  HIP_TRY(hipSetDevice(phys[0]));
  HIP_TRY(c.image.alloc(n_px * 3 * sizeof(float)));
  HIP_TRY(c.image8.alloc(n_px * 3));
  if (G > 1 || force_comm)
  {
    HIP_TRY(c.all_tiles.alloc(n_tiles * TILE_VALS * sizeof(float)));
    HIP_TRY(c.all_tiles8.alloc(n_tiles * TILE_VALS));
  }
  if (c.n_phys > 1 || force_comm)
  {
    std::vector<int> ids(c.n_phys);
    for (int g = 0; g < G; g++)
      if (c.lead[g] == g)
        ids[c.comm_of[g]] = phys[g];
    NCCL_TRY(ncclCommInitAll(c.comms.data(), c.n_phys, ids.data()));
  }
  c.G = G;
  c.W = W;
  c.H = H;
  c.force_comm = force_comm;
  c.bvh_builder = g_bvh_builder;
  scene_serialise(c.scene_bytes, spheres, n_spheres, meshes, n_meshes);
  return RT_HIP_OK;
}

/* ---- launch every device's share; -> *cancelled: the cancel flag was found set between two slabs ---- */
int image_launch_shares(ImageCtx &c, const RtHipCamera *camera, const RtHipParams *params, bool *cancelled)
{
  const int G = c.G;
  for (int g = 0; g < G; g++)
  {
    ImageCtx::Dev &d = c.dev[g];
    HIP_TRY(hipSetDevice(c.phys[g]));
    const size_t slots = d.count ? d.count : 1;
    HIP_TRY(hipMemsetAsync(d.stats.ptr, 0, RT_HIP_NSTATS * sizeof(uint64_t), d.stream));
    HIP_TRY(hipMemsetAsync(d.tiles.ptr, 0, slots * TILE_VALS * sizeof(float), d.stream)); /* unrendered tiles stay black, */
    HIP_TRY(hipMemsetAsync(d.tiles8.ptr, 0, slots * TILE_VALS, d.stream));                /* like the reference's memset  */
    HIP_TRY(d.timer.start(d.stream));
  }
  /* Long frames are rendered in slabs (contiguous runs of each device's tile list) so that a
   * cancel request -- the CLI's SIGINT -- is honoured between slabs; what was finished is
   * still gathered and returned (the reference dumps its partial framebuffer on SIGINT,
   * main.c:37-48, from inside the signal handler; this does it from normal context). */
  const double work = (double)c.W * c.H * (double)params->samples;
  const uint32_t n_slabs = g_cancel ? (work > 4e9 ? 16u : (work > 2e8 ? 4u : 1u)) : 1u;
  *cancelled = false;
  for (uint32_t slab = 0; slab < n_slabs && !*cancelled; slab++)
  {
    for (int g = 0; g < G; g++)
    {
      ImageCtx::Dev &d = c.dev[g];
      const uint32_t k0 = (uint32_t)(((uint64_t)d.count * slab) / n_slabs);
      const uint32_t k1 = (uint32_t)(((uint64_t)d.count * (slab + 1)) / n_slabs);
      if (k1 == k0)
        continue;
      HIP_TRY(hipSetDevice(c.phys[g]));
      RtHipParams p = *params;
      p.tile_first = (uint32_t)g + k0 * (uint32_t)G;
      p.tile_stride = (uint32_t)G;
      p.tile_count = k1 - k0;
      const uint32_t chunks = p.integrator == RT_HIP_CAST_RAY ? 1u : rt_hip_suggest_chunks_depth(d.scene, p.tile_count, p.samples, p.max_depth);
      if (chunks > 1 && !d.ws)
        HIP_TRY(d.ws.alloc(rt_hip_scene_chunk_workspace_bytes(d.scene, d.count)));
      const int rc = rt_hip_render_tiles_chunked(d.scene, camera, &p, chunks, d.ws.ptr, d.tiles.at<float>() + k0 * TILE_VALS,
                                                 d.tiles8.at<uint8_t>() + k0 * TILE_VALS, d.stats.at<uint64_t>(), d.stream);
      if (rc)
        return rc;
    }
    if (n_slabs > 1)
    {
      for (int g = 0; g < G; g++)
      {
        HIP_TRY(hipSetDevice(c.phys[g]));
        HIP_TRY(hipStreamSynchronize(c.dev[g].stream));
      }
      *cancelled = g_cancel && *g_cancel != 0;
    }
  }
  for (int g = 0; g < G; g++)
  {
    HIP_TRY(hipSetDevice(c.phys[g]));
    HIP_TRY(c.dev[g].timer.stop(c.dev[g].stream));
    HIP_TRY(hipEventRecord(c.dev[g].done, c.dev[g].stream));
  }
  return RT_HIP_OK;
}

/* logical device g has a segment that must reach the gathered tiles (the root's own never travels, unless force_comm sends it
 * through RCCL) ... and it goes by RCCL, not by a copy on the root's physical device */
bool image_travels(const ImageCtx &c, int g) { return c.dev[g].count && (g != 0 || c.force_comm); }
bool image_by_rccl(const ImageCtx &c, int g) { return c.force_comm || c.phys[g] != c.phys[0]; }

ncclResult_t image_gather_rccl(ImageCtx &c)
{
  ncclResult_t nr = ncclGroupStart();
  for (int g = 0; g < c.G && nr == ncclSuccess; g++)
  {
    if (!image_travels(c, g) || !image_by_rccl(c, g))
      continue;
    ImageCtx::Dev &d = c.dev[g];
    const size_t nf = d.count * TILE_VALS, at = d.first_slot * TILE_VALS;
    const int from = c.comm_of[g];
    hipStream_t send_stream = c.dev[c.lead[g]].stream;
    nr = ncclSend(d.tiles.ptr, nf, ncclFloat, 0, c.comms[from], send_stream);
    if (nr == ncclSuccess) nr = ncclSend(d.tiles8.ptr, nf, ncclUint8, 0, c.comms[from], send_stream);
    if (nr == ncclSuccess) nr = ncclRecv(c.all_tiles.at<float>() + at, nf, ncclFloat, from, c.comms[0], c.dev[0].stream);
    if (nr == ncclSuccess) nr = ncclRecv(c.all_tiles8.at<uint8_t>() + at, nf, ncclUint8, from, c.comms[0], c.dev[0].stream);
  }
  const ncclResult_t ne = ncclGroupEnd();
  return nr == ncclSuccess ? ne : nr;
}

/* ---- gather on logical device 0 (the root): every segment straight to it ----
 * A segment whose sender shares the root's physical device is a device-to-device copy on the root's stream, ordered after
 * the sender's `done` event; any other travels by grouped ncclSend / ncclRecv (point-to-point over xGMI: a gather to one
 * root uses the root's direct links concurrently, there is no ring).  A physical device is ONE RCCL rank however many
 * logical devices it carries: the rank's sends go on its lead's stream, which first waits for the other senders' `done`.
 * force_comm: every segment, the root's own included, goes through RCCL. */
int image_gather(ImageCtx &c)
{
  HIP_TRY(hipSetDevice(c.phys[0]));
  bool any_rccl = false;
  for (int g = 0; g < c.G; g++)
  {
    if (!image_travels(c, g))
      continue;
    ImageCtx::Dev &d = c.dev[g];
    if (image_by_rccl(c, g))
    {
      any_rccl = true;
      if (c.lead[g] != g)
      {
        HIP_TRY(hipSetDevice(c.phys[g]));
        HIP_TRY(hipStreamWaitEvent(c.dev[c.lead[g]].stream, d.done, 0));
      }
    }
    else
    {
      HIP_TRY(hipSetDevice(c.phys[0]));
      HIP_TRY(hipStreamWaitEvent(c.dev[0].stream, d.done, 0));
      const size_t nf = d.count * TILE_VALS, at = d.first_slot * TILE_VALS;
      HIP_TRY(hipMemcpyAsync(c.all_tiles.at<float>() + at, d.tiles.ptr, nf * sizeof(float), hipMemcpyDeviceToDevice, c.dev[0].stream));
      HIP_TRY(hipMemcpyAsync(c.all_tiles8.at<uint8_t>() + at, d.tiles8.ptr, nf, hipMemcpyDeviceToDevice, c.dev[0].stream));
    }
  }
  if (any_rccl)
    NCCL_TRY(image_gather_rccl(c));
  return RT_HIP_OK;
}

/* scatter each device's segment into the row-major image (root), then wait until every stream is idle */
int image_scatter(ImageCtx &c)
{
  HIP_TRY(hipSetDevice(c.phys[0]));
  for (int g = 0; g < c.G; g++)
  {
    if (!c.dev[g].count)
      continue;
    const bool local = !image_travels(c, g); /* the root's own tiles, where they did not travel */
    const float *src = local ? c.dev[0].tiles.at<float>() : c.all_tiles.at<float>() + c.dev[g].first_slot * TILE_VALS;
    const uint8_t *src8 = local ? c.dev[0].tiles8.at<uint8_t>() : c.all_tiles8.at<uint8_t>() + c.dev[g].first_slot * TILE_VALS;
    const int rc = rt_hip_untile(src, src8, c.W, c.H, (uint32_t)g, (uint32_t)c.G, c.dev[g].count, c.image.at<float>(),
                                 c.image8.at<uint8_t>(), c.dev[0].stream);
    if (rc)
      return rc;
  }
  for (int g = 0; g < c.G; g++)
  {
    HIP_TRY(hipSetDevice(c.phys[g]));
    HIP_TRY(hipStreamSynchronize(c.dev[g].stream));
  }
  return RT_HIP_OK;
}

/* the frame, bytes and counters to the host; -> *fail_flags: the status words (did every workgroup find its pool slots?) */
int image_collect(ImageCtx &c, float *h_image_rgb, uint8_t *h_image_rgb8, uint64_t *h_stats, double *kernel_seconds, uint32_t *fail_flags)
{
  const size_t n_px = (size_t)c.W * c.H;
  *fail_flags = 0;
  for (int g = 0; g < c.G; g++)
    if (c.lead[g] == g)
    { /* the status word of each physical device */
      HIP_TRY(hipSetDevice(c.phys[g]));
      uint32_t f = 0;
      const int rc = status_take(c.phys[g], &f);
      if (rc)
        return rc;
      *fail_flags |= f;
    }
  HIP_TRY(hipSetDevice(c.phys[0]));
  if (h_image_rgb)
    HIP_TRY(hipMemcpy(h_image_rgb, c.image.ptr, n_px * 3 * sizeof(float), hipMemcpyDeviceToHost));
  if (h_image_rgb8)
    HIP_TRY(hipMemcpy(h_image_rgb8, c.image8.ptr, n_px * 3, hipMemcpyDeviceToHost));
  double worst = 0;
  uint64_t sums[RT_HIP_NSTATS] = {0, 0, 0, 0};
  for (int g = 0; g < c.G; g++)
  {
    HIP_TRY(hipSetDevice(c.phys[g]));
    float ms = 0;
    HIP_TRY(c.dev[g].timer.elapsed_ms(&ms));
    if (ms * 1e-3 > worst)
      worst = ms * 1e-3;
    uint64_t st[RT_HIP_NSTATS];
    HIP_TRY(hipMemcpy(st, c.dev[g].stats.ptr, sizeof st, hipMemcpyDeviceToHost));
    for (int k = 0; k < RT_HIP_NSTATS; k++)
      sums[k] += st[k];
  }
  if (h_stats)
    memcpy(h_stats, sums, sizeof sums);
  if (kernel_seconds)
    *kernel_seconds = worst;
  return RT_HIP_OK;
}

int render_image_impl(const RtHipSphere *spheres, size_t n_spheres, const RtHipMesh *meshes, size_t n_meshes,
                      const RtHipCamera *camera, const RtHipParams *params, int n_devices, float *h_image_rgb,
                      uint8_t *h_image_rgb8, uint64_t *h_stats, double *kernel_seconds)
{
  int rc = check_params(params);
  if (rc)
    return rc;
  if (!camera)
    return fail(RT_HIP_EINVAL, "camera is NULL");
  const int have = usable_devices();
  if (have < 1)
    return fail(RT_HIP_ENODEV, "no HIP device is available (this library has no CPU path)");
  const int W = params->width, H = params->height;
  std::lock_guard<std::mutex> lock(g_ctx_mutex); /* one frame at a time: the context is shared */
  device_map_from_env();
  const int limit = g_device_map.empty() ? have : (int)g_device_map.size();
  if (n_devices < 1 || n_devices > limit)
    return fail(RT_HIP_ENODEV, "asked for %d devices, %d available%s", n_devices, limit, g_device_map.empty() ? "" : " in the device map");
  const int G = n_devices;
  std::vector<int> phys(G);
  for (int g = 0; g < G; g++)
  {
    phys[g] = g_device_map.empty() ? g : g_device_map[g];
    if (phys[g] < 0 || phys[g] >= have)
      return fail(RT_HIP_ENODEV, "device map entry %d -> %d: %d devices available", g, phys[g], have);
  }
  const auto tick0 = std::chrono::steady_clock::now();
  CtxGuard guard; /* from here on a failure drops the cached context */
  rc = ctx_prepare(spheres, n_spheres, meshes, n_meshes, G, phys, W, H);
  if (rc)
    return rc;
  const auto tick1 = std::chrono::steady_clock::now();
  ImageCtx &c = g_ctx;
  bool cancelled = false;
  rc = image_launch_shares(c, camera, params, &cancelled);
  if (!rc)
    rc = image_gather(c);
  if (!rc)
    rc = image_scatter(c);
  if (rc)
    return rc;
  const auto tick2 = std::chrono::steady_clock::now();
  uint32_t fail_flags = 0;
  rc = image_collect(c, h_image_rgb, h_image_rgb8, h_stats, kernel_seconds, &fail_flags);
  if (rc)
    return rc;
  guard.keep(); /* a status word or a cancel request is the frame's result: the context is sound */
  {
    const auto tick3 = std::chrono::steady_clock::now();
    auto secs = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) {
      return std::chrono::duration<double>(b - a).count();
    };
    g_last_phases[0] = secs(tick0, tick1); /* context: scene compare, or upload + buffers + workspaces + communicators */
    g_last_phases[1] = secs(tick1, tick2); /* launches, kernels, gather, scatter -- until every stream is idle */
    g_last_phases[2] = secs(tick2, tick3); /* the frame, bytes and counters over PCIe */
  }
  if (fail_flags)
    return status_to_error(fail_flags); /* the buffers hold what was rendered; the unrendered tiles read NaN / 255 */
  if (cancelled)
    return fail(RT_HIP_ECANCELLED, "render cancelled: the image holds the tiles finished so far");
  return RT_HIP_OK;
}

int set_device_map_impl(const int *map, int n)
{
  if (n < 0 || n > 64 || (n > 0 && !map))
    return fail(RT_HIP_EINVAL, "device map: 0 <= n <= 64 entries");
  const int have = usable_devices();
  for (int k = 0; k < n; k++)
    if (map[k] < 0 || map[k] >= have)
      return fail(RT_HIP_ENODEV, "device map entry %d -> %d: %d devices available", k, map[k], have);
  std::lock_guard<std::mutex> lock(g_ctx_mutex);
  g_device_map_env_read = true; /* an explicit map (or its removal) overrides RT_HIP_DEVICE_MAP */
  g_device_map.assign(map, map + n);
  return RT_HIP_OK;
}

void last_phases_impl(double out[3])
{
  std::lock_guard<std::mutex> lock(g_ctx_mutex);
  memcpy(out, g_last_phases, sizeof g_last_phases);
}

void release_cache_impl()
{
  {
    std::lock_guard<std::mutex> lock(g_ctx_mutex);
    ctx_release(g_ctx);
  }
  pend_pools_release();
  grid_tail_release();
}

int set_bvh_builder_impl(int builder)
{
  if (builder != RT_HIP_BVH_HOST && builder != RT_HIP_BVH_DEVICE)
    return fail(RT_HIP_EINVAL, "bvh builder %d: RT_HIP_BVH_HOST (0) or RT_HIP_BVH_DEVICE (1)", builder);
  std::lock_guard<std::mutex> lock(g_ctx_mutex);
  g_bvh_builder = builder;
  return RT_HIP_OK;
}

uint64_t cache_builds_impl()
{
  std::lock_guard<std::mutex> lock(g_ctx_mutex);
  return g_ctx.builds;
}

uint64_t cache_updates_impl()
{
  std::lock_guard<std::mutex> lock(g_ctx_mutex);
  return g_ctx.updates;
}

void set_scene_updates_impl(int on)
{
  std::lock_guard<std::mutex> lock(g_ctx_mutex);
  g_scene_updates = on != 0;
}

void set_material_updates_impl(int on)
{
  std::lock_guard<std::mutex> lock(g_ctx_mutex);
  g_material_updates = on != 0;
}

int set_bvh_rebuild_ratio_impl(double max_ratio)
{
  if (!(max_ratio == 0.0 || (max_ratio >= 1.0 && max_ratio < HUGE_VAL)))
    return fail(RT_HIP_EINVAL, "bvh rebuild ratio: 0 (never rebuild) or a finite ratio >= 1");
  std::lock_guard<std::mutex> lock(g_ctx_mutex);
  g_bvh_rebuild_ratio = max_ratio == 0.0 ? 0.0 : max_ratio;
  return RT_HIP_OK;
}

uint64_t cache_rebuilds_impl()
{
  std::lock_guard<std::mutex> lock(g_ctx_mutex);
  return g_ctx.rebuilds;
}

/* logical device `device` of the device map (the HIP device itself without a map) -> the HIP device, or RT_HIP_ENODEV */
int physical_device(int device, int *phys)
{
  const int have = usable_devices();
  if (have < 1)
    return fail(RT_HIP_ENODEV, "no HIP device is available (this library has no CPU path)");
  *phys = device;
  {
    std::lock_guard<std::mutex> lock(g_ctx_mutex);
    device_map_from_env();
    if (!g_device_map.empty())
    {
      if (device < 0 || device >= (int)g_device_map.size())
        return fail(RT_HIP_ENODEV, "logical device %d: the device map has %d entries", device, (int)g_device_map.size());
      *phys = g_device_map[device];
    }
  }
  if (*phys < 0 || *phys >= have)
    return fail(RT_HIP_ENODEV, "no HIP device %d", *phys);
  return RT_HIP_OK;
}

/* the device that holds `ptr`: a host pointer would fault the kernel, so it is refused */
int device_of(const void *ptr, const char *what, int *device)
{
  if (usable_devices() < 1)
    return fail(RT_HIP_ENODEV, "no HIP device is available (this library has no CPU path)");
  hipPointerAttribute_t attr = {};
  if (hipPointerGetAttributes(&attr, ptr) != hipSuccess || attr.type != hipMemoryTypeDevice)
  {
    (void)hipGetLastError();
    return fail(RT_HIP_EINVAL, "%s is not device memory", what);
  }
  *device = attr.device;
  return RT_HIP_OK;
}

/* The prologues of the calls that are given no scene: `body` runs with a device current -- the one that holds `ptr` (a
 * device-pointer form), or logical device `device` of the device map (a host-array form; body(phys) gets the HIP device; a host
 * form that is given a scene's primitives gets body(scene, phys): a scene of the call's own on that device, destroyed on return) --
 * and the previous device comes back when it returns.  A lookup or a scene that fails is the call's answer and `body` does not run. */
template <class F>
int on_device_of(const void *ptr, const char *what, F &&body)
{
  int device = -1;
  if (const int rc = device_of(ptr, what, &device))
    return rc;
  DeviceScope scope(device);
  HIP_TRY(scope.status);
  return body();
}

template <class F>
int on_logical_device(int device, F &&body)
{
  int phys = -1;
  if (const int rc = physical_device(device, &phys))
    return rc;
  DeviceScope scope(phys);
  HIP_TRY(scope.status);
  return body(phys);
}

template <class F>
int with_owned_scene(const RtHipSphere *spheres, size_t n_spheres, const RtHipMesh *meshes, size_t n_meshes, int device, F &&body)
{
  int phys = -1;
  if (const int rc = physical_device(device, &phys))
    return rc;
  OwnedScene own;
  if (const int rc = own.create(spheres, n_spheres, meshes, n_meshes, phys))
    return rc;
  DeviceScope scope(phys);
  HIP_TRY(scope.status);
  return body(own.scene, phys);
}

/* rt_hip_render_aov_image on its scene, the scene's device current: compact buffers for the requested outputs, one launch over
 * every tile, the scatter, the copies.  Synchronous on the null stream. */
int aov_image_of(const RtHipScene *scene, const RtHipCamera *camera, const RtHipParams *params, const RtHipAov *h_image)
{
  RtHipParams p = *params;
  whole_image(p);
  const size_t tile_px = (size_t)p.tile_count * PT_TILE_PIXELS, img_px = (size_t)p.width * p.height;
  /* per requested output its tile buffer and its image, 32-bit words */
  void *host[5] = {h_image->albedo, h_image->normal, h_image->depth, h_image->object, h_image->hits};
  StageArena A;
  int tp[5], ip[5];
  for (int k = 0; k < 5; k++)
  {
    const size_t px_bytes = (k < 2 ? 3u : 1u) * sizeof(uint32_t);
    tp[k] = A.part(px_bytes * tile_px, nullptr, nullptr, host[k] != nullptr);
    ip[k] = A.part(px_bytes * img_px, nullptr, host[k], host[k] != nullptr);
  }
  int rc = A.stage();
  if (rc)
    return rc;
  const RtHipAov tiles = {A.at<float>(tp[0]), A.at<float>(tp[1]), A.at<float>(tp[2]), A.at<uint32_t>(tp[3]), A.at<uint32_t>(tp[4])};
  const RtHipAov image = {A.at<float>(ip[0]), A.at<float>(ip[1]), A.at<float>(ip[2]), A.at<uint32_t>(ip[3]), A.at<uint32_t>(ip[4])};
  rc = rt_hip_render_aov_tiles(scene, camera, &p, &tiles, nullptr);
  if (!rc)
    rc = rt_hip_untile_aov(&tiles, p.width, p.height, 0, 1, p.tile_count, &image, nullptr);
  return rc ? rc : A.download();
}

/* ... with a scene of its own on the logical device */
int render_aov_image_impl(const RtHipSphere *spheres, size_t n_spheres, const RtHipMesh *meshes, size_t n_meshes,
                          const RtHipCamera *camera, const RtHipParams *params, int device, const RtHipAov *h_image)
{
  if (!camera || !params)
    return fail(RT_HIP_EINVAL, "camera and params are required");
  if (!aov_any(h_image))
    return fail(RT_HIP_EINVAL, "h_image: at least one output array is required");
  if (const int rc = check_params(params))
    return rc;
  return with_owned_scene(spheres, n_spheres, meshes, n_meshes, device,
                          [&](const RtHipScene *scene, int) { return aov_image_of(scene, camera, params, h_image); });
}

/* ---- the denoiser (rt_hip.h, rt_hip_denoise_*) ------------------------------------------------------------------------------
 * Workspace layout for n = w*h pixels, each part 256-B aligned: e[0], e[1] and the guidance (16 B per pixel each), then hits +
 * object (8 B per pixel).  The kernels and their arithmetic are pt_denoise_* in image_ops.hip. */
/* a frame of the image-space calls: both sides in [min_side, 2^20], fewer than 2^32 pixels */
bool frame_size_ok(int32_t width, int32_t height, int32_t min_side)
{
  return width >= min_side && height >= min_side && width <= (1 << 20) && height <= (1 << 20) &&
         (uint64_t)width * (uint64_t)height <= 0xFFFFFFFFull;
}

size_t denoise_ws_bytes(size_t n) { return 3u * stage_align(16u * n) + stage_align(8u * n); }

int check_denoise(const float *rgb, const RtHipAov *aov, int32_t width, int32_t height, const RtHipDenoiseParams *p, const void *out_rgb,
                  const void *out_rgb8)
{
  if (!p)
    return fail(RT_HIP_EINVAL, "params is NULL");
  if (!frame_size_ok(width, height, 1))
    return fail(RT_HIP_EINVAL, "width and height must be in [1, 2^20] with fewer than 2^32 pixels");
  if (p->iterations < 0 || p->iterations > 10)
    return fail(RT_HIP_EINVAL, "iterations must be in [0, 10]");
  if (p->normal_power_log2 > 10)
    return fail(RT_HIP_EINVAL, "normal_power_log2 must be in [0, 10]");
  if (p->flags & ~(uint32_t)(RT_HIP_DENOISE_DEMODULATE | RT_HIP_DENOISE_OBJECT_EDGES))
    return fail(RT_HIP_EINVAL, "unknown denoise flags 0x%x", p->flags);
  if (!(std::isfinite(p->sigma_color) && p->sigma_color > 0) || !(std::isfinite(p->sigma_depth) && p->sigma_depth > 0))
    return fail(RT_HIP_EINVAL, "sigma_color and sigma_depth must be finite and > 0");
  if (!rgb)
    return fail(RT_HIP_EINVAL, "the colour image is required");
  if (!aov || !aov->normal || !aov->depth || !aov->hits)
    return fail(RT_HIP_EINVAL, "the normal, depth and hits buffers are required");
  if ((p->flags & RT_HIP_DENOISE_DEMODULATE) && !aov->albedo)
    return fail(RT_HIP_EINVAL, "RT_HIP_DENOISE_DEMODULATE needs the albedo buffer");
  if ((p->flags & RT_HIP_DENOISE_OBJECT_EDGES) && !aov->object)
    return fail(RT_HIP_EINVAL, "RT_HIP_DENOISE_OBJECT_EDGES needs the object buffer");
  if (!out_rgb && !out_rgb8)
    return fail(RT_HIP_EINVAL, "at least one output is required");
  return RT_HIP_OK;
}

/* the launches of a checked call, on the current device */
int denoise_launch(const float *rgb, const RtHipAov *aov, int32_t width, int32_t height, const RtHipDenoiseParams *p, void *ws,
                   float *out_rgb, uint8_t *out_rgb8, hipStream_t stream)
{
  const size_t n = (size_t)width * (size_t)height, part = stage_align(16u * n);
  char *w = static_cast<char *>(ws);
  PtDenoise D = {};
  D.rgb = rgb;
  D.albedo = aov->albedo;
  D.normal = aov->normal;
  D.depth = aov->depth;
  D.hits = aov->hits;
  D.object = aov->object;
  D.e[0] = reinterpret_cast<float *>(w);
  D.e[1] = reinterpret_cast<float *>(w + part);
  D.guide = reinterpret_cast<float *>(w + 2u * part);
  D.hit_obj = reinterpret_cast<uint32_t *>(w + 3u * part);
  D.out_rgb = out_rgb;
  D.out_rgb8 = out_rgb8;
  D.width = width;
  D.height = height;
  D.demodulate = (p->flags & RT_HIP_DENOISE_DEMODULATE) ? 1u : 0u;
  D.object_edges = (p->flags & RT_HIP_DENOISE_OBJECT_EDGES) ? 1u : 0u;
  D.k = p->normal_power_log2;
  D.sigma_z = p->sigma_depth;
  return launched(pt_launch_denoise(D, p->iterations, p->sigma_color, stream), "pt_denoise");
}

int denoise_image_impl(const float *h_rgb, const RtHipAov *h_aov, int32_t width, int32_t height, const RtHipDenoiseParams *params,
                       int device, float *h_out, uint8_t *h_out8)
{
  if (const int rc = check_denoise(h_rgb, h_aov, width, height, params, h_out, h_out8))
    return rc;
  return on_logical_device(device, [&](int) {
    const size_t n = (size_t)width * (size_t)height;
    const bool demod = (params->flags & RT_HIP_DENOISE_DEMODULATE) != 0, edges = (params->flags & RT_HIP_DENOISE_OBJECT_EDGES) != 0;
    /* the workspace, the colour (in and out: the floats are filtered in place), the buffers the flags ask for, the bytes */
    StageArena A;
    const int ws = A.part(denoise_ws_bytes(n));
    const int rgb = A.part(12u * n, h_rgb, h_out);
    const AovStage aov(A, h_aov, n, demod, edges);
    const int rgb8 = A.part(3u * n, nullptr, h_out8, h_out8 != nullptr);
    int rc = A.stage();
    if (rc)
      return rc;
    const RtHipAov d = aov.device(A);
    rc = denoise_launch(A.at<float>(rgb), &d, width, height, params, A.at<char>(ws), h_out ? A.at<float>(rgb) : nullptr,
                        A.at<uint8_t>(rgb8), nullptr);
    return rc ? rc : A.download();
  });
}

/* ---- temporal reprojection (rt_hip.h, rt_hip_reproject*) ---------------------------------------------------------------------
 * One launch of pt_reproject (image_ops.hip), no workspace.  The arguments that need no device are checked first. */
bool ranges_overlap(const void *a, size_t a_bytes, const void *b, size_t b_bytes)
{
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
  return a && b && a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

/* The overlap rule of the image-space calls, whose lanes write their outputs while other lanes still read: output by output, in
 * the order given, first against every input (`in_text`), then against the outputs after it (`out_text`; null: they are not
 * compared).  One pair may be in place -- outs[place_out] and ins[place_in] at the SAME address, where a lane reads its own
 * element before it writes it; -1: none.  A null span is absent and overlaps nothing. */
struct Span
{
  const void *ptr;
  size_t bytes;
};

template <size_t N_OUT, size_t N_IN>
int check_overlap(const Span (&outs)[N_OUT], const Span (&ins)[N_IN], int place_out, int place_in, const char *in_text, const char *out_text)
{
  for (size_t o = 0; o < N_OUT; o++)
  {
    for (size_t i = 0; i < N_IN; i++)
      if (!((int)o == place_out && (int)i == place_in && outs[o].ptr == ins[i].ptr) &&
          ranges_overlap(outs[o].ptr, outs[o].bytes, ins[i].ptr, ins[i].bytes))
        return fail(RT_HIP_EINVAL, "%s", in_text);
    for (size_t q = o + 1; out_text && q < N_OUT; q++)
      if (ranges_overlap(outs[o].ptr, outs[o].bytes, outs[q].ptr, outs[q].bytes))
        return fail(RT_HIP_EINVAL, "%s", out_text);
  }
  return RT_HIP_OK;
}

int check_reproject(const float *rgb, const RtHipAov *aov, const RtHipCamera *camera, const float *hist_rgb, const float *hist_len,
                    const RtHipAov *hist_aov, const RtHipCamera *hist_camera, int32_t width, int32_t height,
                    const RtHipReprojectParams *p, const float *out_rgb, const uint8_t *out_rgb8, const float *out_len,
                    const float *out_motion)
{
  if (!p)
    return fail(RT_HIP_EINVAL, "params is NULL");
  if (!frame_size_ok(width, height, 2))
    return fail(RT_HIP_EINVAL, "width and height must be in [2, 2^20] with fewer than 2^32 pixels");
  if (p->flags != 0u)
    return fail(RT_HIP_EINVAL, "unknown reproject flags 0x%x", p->flags);
  if (!(std::isfinite(p->max_history) && p->max_history >= 1.0))
    return fail(RT_HIP_EINVAL, "max_history must be finite and >= 1");
  if (!(std::isfinite(p->depth_tol) && p->depth_tol >= 0.0))
    return fail(RT_HIP_EINVAL, "depth_tol must be finite and >= 0");
  if (!std::isfinite(p->normal_min))
    return fail(RT_HIP_EINVAL, "normal_min must be finite");
  if (!rgb || !camera)
    return fail(RT_HIP_EINVAL, "the colour image and the camera are required");
  if (!aov || !aov->normal || !aov->depth || !aov->hits || !aov->object)
    return fail(RT_HIP_EINVAL, "the normal, depth, hits and object buffers are required");
  const bool any_hist = hist_rgb || hist_len || hist_aov || hist_camera;
  if (any_hist && !(hist_rgb && hist_len && hist_aov && hist_camera))
    return fail(RT_HIP_EINVAL, "the history's colour, length, buffers and camera are given together or not at all");
  if (any_hist && (!hist_aov->normal || !hist_aov->depth || !hist_aov->hits || !hist_aov->object))
    return fail(RT_HIP_EINVAL, "the history's normal, depth, hits and object buffers are required");
  if (!out_rgb || !out_len)
    return fail(RT_HIP_EINVAL, "out_rgb and out_len are required");
  /* a lane writes its pixel's outputs while other lanes still read: no output may overlap what the call reads (the history, the
   * frame's buffers) or another output; only out_rgb == rgb, where a lane reads its own pixel before it writes it, is in place */
  const size_t n = (size_t)width * (size_t)height;
  const Span outs[4] = {{out_rgb, 12u * n}, {out_rgb8, 3u * n}, {out_len, 4u * n}, {out_motion, 8u * n}};
  const Span frame[5] = {{rgb, 12u * n}, {aov->normal, 12u * n}, {aov->depth, 4u * n}, {aov->hits, 4u * n}, {aov->object, 4u * n}};
  if (const int rc = check_overlap(outs, frame, 0, 0, "an output overlaps a buffer of the frame (only out_rgb == rgb is allowed)",
                                   "two outputs overlap"))
    return rc;
  if (!any_hist)
    return RT_HIP_OK;
  const Span hist[6] = {{hist_rgb, 12u * n},        {hist_len, 4u * n},       {hist_aov->normal, 12u * n},
                        {hist_aov->depth, 4u * n}, {hist_aov->hits, 4u * n}, {hist_aov->object, 4u * n}};
  return check_overlap(outs, hist, -1, -1, "an output aliases a history buffer", nullptr);
}

void camera_of(const RtHipCamera *c, PtCamera &out)
{
  for (int k = 0; k < 3; k++)
  {
    out.pos[k] = c->position[k];
    out.horizontal[k] = c->horizontal[k];
    out.vertical[k] = c->vertical[k];
    out.llc[k] = c->lower_left_corner[k];
  }
}

/* the launch of a checked call, on the current device */
int reproject_launch(const float *rgb, const RtHipAov *aov, const RtHipCamera *camera, const float *hist_rgb, const float *hist_len,
                     const RtHipAov *hist_aov, const RtHipCamera *hist_camera, int32_t width, int32_t height,
                     const RtHipReprojectParams *p, const double *prev_points, float *out_rgb, uint8_t *out_rgb8, float *out_len,
                     float *out_motion, hipStream_t stream)
{
  PtReproject R = {};
  R.rgb = rgb;
  R.normal = aov->normal;
  R.depth = aov->depth;
  R.hits = aov->hits;
  R.object = aov->object;
  camera_of(camera, R.cam);
  if (hist_rgb)
  {
    R.hist_rgb = hist_rgb;
    R.hist_len = hist_len;
    R.hist_normal = hist_aov->normal;
    R.hist_depth = hist_aov->depth;
    R.hist_hits = hist_aov->hits;
    R.hist_object = hist_aov->object;
    camera_of(hist_camera, R.hist_cam);
  }
  R.out_rgb = out_rgb;
  R.out_rgb8 = out_rgb8;
  R.out_len = out_len;
  R.out_motion = out_motion;
  R.width = width;
  R.height = height;
  R.max_history = p->max_history;
  R.depth_tol = p->depth_tol;
  R.normal_min = p->normal_min;
  return prev_points ? launched(pt_launch_reproject_points(R, prev_points, stream), "pt_reproject_points")
                     : launched(pt_launch_reproject(R, stream), "pt_reproject");
}

/* rt_hip_reproject_points' own rule, after check_reproject's: the previous points (3 doubles per pixel) overlap no output */
int check_reproject_points(const double *prev_points, int32_t width, int32_t height, const float *out_rgb, const uint8_t *out_rgb8,
                           const float *out_len, const float *out_motion)
{
  const size_t n = (size_t)width * (size_t)height;
  const Span outs[4] = {{out_rgb, 12u * n}, {out_rgb8, 3u * n}, {out_len, 4u * n}, {out_motion, 8u * n}};
  const Span points[1] = {{prev_points, 24u * n}};
  return check_overlap(outs, points, -1, -1, "an output overlaps the previous points", nullptr);
}

int reproject_image_impl(const float *h_rgb, const RtHipAov *h_aov, const RtHipCamera *camera, const float *h_hist_rgb,
                         const float *h_hist_len, const RtHipAov *h_hist_aov, const RtHipCamera *hist_camera, int32_t width,
                         int32_t height, const RtHipReprojectParams *params, const double *h_prev_points, int device, float *h_out_rgb,
                         uint8_t *h_out_rgb8, float *h_out_len, float *h_out_motion)
{
  int rc = check_reproject(h_rgb, h_aov, camera, h_hist_rgb, h_hist_len, h_hist_aov, hist_camera, width, height, params, h_out_rgb,
                           h_out_rgb8, h_out_len, h_out_motion);
  if (!rc && h_prev_points)
    rc = check_reproject_points(h_prev_points, width, height, h_out_rgb, h_out_rgb8, h_out_len, h_out_motion);
  if (rc)
    return rc;
  return on_logical_device(device, [&](int) {
    const size_t n = (size_t)width * (size_t)height;
    const bool hist = h_hist_rgb != nullptr;
    /* per image -- the frame, then the history if there is one -- colour, normal, depth, hits, object and length: the frame's
     * colour and length are the outputs (the colour in place); then motion and bytes */
    const RtHipAov none = {};
    StageArena A;
    const int rgb = A.part(12u * n, h_rgb, h_out_rgb);
    const AovStage aov(A, h_aov, n, false, true);
    const int len = A.part(4u * n, nullptr, h_out_len);
    const int hist_rgb = A.part(12u * n, h_hist_rgb, nullptr, hist);
    const AovStage hist_aov(A, hist ? h_hist_aov : &none, n, false, true, hist);
    const int hist_len = A.part(4u * n, h_hist_len, nullptr, hist);
    const int motion = A.part(8u * n, nullptr, h_out_motion, h_out_motion != nullptr);
    const int rgb8 = A.part(3u * n, nullptr, h_out_rgb8, h_out_rgb8 != nullptr);
    const int points = A.part(24u * n, h_prev_points, nullptr, h_prev_points != nullptr);
    int rc = A.stage();
    if (rc)
      return rc;
    const RtHipAov d_aov = aov.device(A), d_hist_aov = hist_aov.device(A);
    rc = reproject_launch(A.at<float>(rgb), &d_aov, camera, A.at<float>(hist_rgb), A.at<float>(hist_len), hist ? &d_hist_aov : nullptr,
                          hist_camera, width, height, params, A.at<double>(points), A.at<float>(rgb), A.at<uint8_t>(rgb8),
                          A.at<float>(len), A.at<float>(motion), nullptr);
    return rc ? rc : A.download();
  });
}

/* ---- previous points (rt_hip.h, rt_hip_prev_points*, rt_hip_prev_points_moved*) ------------------------------------------------
 * One launch of pt_prev_points, or of pt_prev_points_moved for a call that takes spheres (image_ops.hip), no workspace.  One path
 * for both: `spheres` is null for rt_hip_prev_points and the call's sphere arguments for rt_hip_prev_points_moved.  The arguments
 * that need no device are checked first: the common ones, then the spheres' -- object is required, and both sphere arrays with a
 * non-zero count. */
struct MovedSpheres
{
  const double *prev, *cur; /* 4 doubles per sphere; null with n == 0 */
  size_t n;
  bool none_given; /* no previous spheres and n == 0: no sphere moved (PtPrevPointsMoved.spheres_static) -- by the CALL's pointers */
};

MovedSpheres moved_spheres(const double *prev, const double *cur, size_t n) { return {prev, cur, n, !prev && n == 0}; }

int check_prev_points(const RtHipHits *hits, uint64_t n, const double *positions, size_t n_triangles, const MovedSpheres *spheres,
                      const double *points)
{
  if (n >= (1ull << 32))
    return fail(RT_HIP_EINVAL, "n must be below 2^32");
  if (n_triangles > SIZE_MAX / 72u)
    return fail(RT_HIP_EINVAL, "n_triangles is out of range");
  if (!hits || !hits->status || !hits->prim || !hits->bary || !hits->point)
    return fail(RT_HIP_EINVAL, "the hits' status, prim, bary and point are required");
  if (n_triangles && !positions)
    return fail(RT_HIP_EINVAL, "the previous positions are required (9 doubles per triangle)");
  if (!points)
    return fail(RT_HIP_EINVAL, "the output points are required");
  /* a lane writes its entry while other lanes still read: the output overlaps no input, but for out == point, where a lane reads
   * its own point before it writes it */
  const char *text = "the output overlaps an input (only d_points == d_hits->point is allowed)";
  const Span out[1] = {{points, 24u * n}};
  const Span in[5] = {{hits->status, 4u * n}, {hits->prim, 4u * n}, {hits->bary, 16u * n}, {hits->point, 24u * n},
                      {n_triangles ? positions : nullptr, 72u * n_triangles}};
  if (const int rc = check_overlap(out, in, 0, 3, text, nullptr))
    return rc;
  if (!spheres)
    return RT_HIP_OK;
  if (!hits->object)
    return fail(RT_HIP_EINVAL, "the hits' object is required");
  if (spheres->n > SIZE_MAX / 32u)
    return fail(RT_HIP_EINVAL, "n_spheres is out of range");
  if (spheres->n && (!spheres->prev || !spheres->cur))
    return fail(RT_HIP_EINVAL, "the previous and the current spheres are required (4 doubles per sphere)");
  const Span moved[3] = {{hits->object, 4u * n}, {spheres->n ? spheres->prev : nullptr, 32u * spheres->n},
                         {spheres->n ? spheres->cur : nullptr, 32u * spheres->n}};
  return check_overlap(out, moved, -1, -1, text, nullptr);
}

/* the launch of a checked call, on the current device */
int prev_points_launch(const RtHipHits *hits, uint64_t n, const double *positions, size_t n_triangles, const MovedSpheres *spheres,
                       double *points, hipStream_t stream)
{
  if (n == 0)
    return RT_HIP_OK;
  if (spheres)
  {
    const PtPrevPointsMoved A = {.status = hits->status, .prim = hits->prim, .object = hits->object, .bary = hits->bary, .point = hits->point,
                                 .positions = positions, .spheres_prev = spheres->prev, .spheres_cur = spheres->cur, .out = points, .n = n,
                                 .n_triangles = n_triangles, .n_spheres = spheres->n, .spheres_static = spheres->none_given ? 1u : 0u};
    return launched(pt_launch_prev_points_moved(A, stream), "pt_prev_points_moved");
  }
  const PtPrevPoints A = {.status = hits->status, .prim = hits->prim, .bary = hits->bary, .point = hits->point, .positions = positions,
                          .out = points, .n = n, .n_triangles = n_triangles};
  return launched(pt_launch_prev_points(A, stream), "pt_prev_points");
}

/* the device-pointer form: no entry returns before a device is looked for */
int prev_points_device(const RtHipHits *d_hits, uint64_t n, const double *d_positions, size_t n_triangles, const MovedSpheres *spheres,
                       double *d_points, void *stream)
{
  const int rc = check_prev_points(d_hits, n, d_positions, n_triangles, spheres, d_points);
  if (rc || n == 0)
    return rc;
  return on_device_of(d_points, "d_points", [&] {
    return prev_points_launch(d_hits, n, d_positions, n_triangles, spheres, d_points, static_cast<hipStream_t>(stream));
  });
}

/* the host-array form: the logical device is looked up before no entry returns */
int prev_points_host_impl(const RtHipHits *h_hits, uint64_t n, const double *h_positions, size_t n_triangles, const MovedSpheres *spheres,
                          int device, double *h_points)
{
  if (const int rc = check_prev_points(h_hits, n, h_positions, n_triangles, spheres, h_points))
    return rc;
  return on_logical_device(device, [&](int) -> int {
    if (n == 0)
      return RT_HIP_OK;
    /* the point part is input and output: the kernel runs in place on it */
    const size_t n_spheres = spheres ? spheres->n : 0;
    StageArena A;
    const int status = A.part(4u * n, h_hits->status);
    const int prim = A.part(4u * n, h_hits->prim);
    const int object = A.part(4u * n, h_hits->object, nullptr, spheres != nullptr);
    const int bary = A.part(16u * n, h_hits->bary);
    const int point = A.part(24u * n, h_hits->point, h_points);
    const int positions = A.part(72u * n_triangles, h_positions, nullptr, n_triangles != 0);
    const int sprev = A.part(32u * n_spheres, spheres ? spheres->prev : nullptr, nullptr, n_spheres != 0);
    const int scur = A.part(32u * n_spheres, spheres ? spheres->cur : nullptr, nullptr, n_spheres != 0);
    int rc = A.stage();
    if (rc)
      return rc;
    const RtHipHits d = {A.at<uint32_t>(status), nullptr, A.at<uint32_t>(object), A.at<uint32_t>(prim), A.at<double>(point), nullptr, A.at<double>(bary), nullptr};
    const MovedSpheres d_spheres = {A.at<double>(sprev), A.at<double>(scur), n_spheres, spheres && spheres->none_given};
    rc = prev_points_launch(&d, n, A.at<double>(positions), n_triangles, spheres ? &d_spheres : nullptr, A.at<double>(point), nullptr);
    return rc ? rc : A.download();
  });
}

/* ---- guided upsampling (rt_hip.h, rt_hip_upsample*) ---------------------------------------------------------------------------
 * One launch of pt_upsample (image_ops.hip), no workspace.  The arguments that need no device are checked first. */
int check_upsample(const float *low_rgb, const RtHipAov *low_aov, int32_t low_width, int32_t low_height, const RtHipAov *aov,
                   int32_t width, int32_t height, const RtHipUpsampleParams *p, const float *out_rgb, const uint8_t *out_rgb8,
                   const float *out_conf)
{
  if (!p)
    return fail(RT_HIP_EINVAL, "params is NULL");
  if (!frame_size_ok(width, height, 2) || !frame_size_ok(low_width, low_height, 2))
    return fail(RT_HIP_EINVAL, "the widths and heights must be in [2, 2^20] with fewer than 2^32 pixels per frame");
  if (p->flags & ~(uint32_t)(RT_HIP_UPSAMPLE_DEMODULATE | RT_HIP_UPSAMPLE_OBJECT_EDGES))
    return fail(RT_HIP_EINVAL, "unknown upsample flags 0x%x", p->flags);
  if (p->normal_power_log2 > 10u)
    return fail(RT_HIP_EINVAL, "normal_power_log2 must be 0 .. 10");
  if (!(std::isfinite(p->sigma_depth) && p->sigma_depth > 0.0))
    return fail(RT_HIP_EINVAL, "sigma_depth must be finite and > 0");
  if (!low_rgb || !low_aov || !aov)
    return fail(RT_HIP_EINVAL, "the low frame's colour and the buffers of both frames are required");
  const bool demod = (p->flags & RT_HIP_UPSAMPLE_DEMODULATE) != 0u, edges = (p->flags & RT_HIP_UPSAMPLE_OBJECT_EDGES) != 0u;
  for (const RtHipAov *a : {low_aov, aov})
  {
    if (!a->normal || !a->depth || !a->hits)
      return fail(RT_HIP_EINVAL, "the normal, depth and hits buffers of both frames are required");
    if (demod && !a->albedo)
      return fail(RT_HIP_EINVAL, "RT_HIP_UPSAMPLE_DEMODULATE needs the albedo buffers of both frames");
    if (edges && !a->object)
      return fail(RT_HIP_EINVAL, "RT_HIP_UPSAMPLE_OBJECT_EDGES needs the object buffers of both frames");
  }
  if (!out_rgb)
    return fail(RT_HIP_EINVAL, "out_rgb is required");
  /* a lane writes its pixel while other lanes still read the low frame: no output may overlap what the call reads or another output */
  const size_t n = (size_t)width * (size_t)height, nl = (size_t)low_width * (size_t)low_height;
  const Span outs[3] = {{out_rgb, 12u * n}, {out_rgb8, 3u * n}, {out_conf, 4u * n}};
  const Span ins[11] = {{low_rgb, 12u * nl},
                        {demod ? low_aov->albedo : nullptr, 12u * nl},
                        {low_aov->normal, 12u * nl},
                        {low_aov->depth, 4u * nl},
                        {low_aov->hits, 4u * nl},
                        {edges ? low_aov->object : nullptr, 4u * nl},
                        {demod ? aov->albedo : nullptr, 12u * n},
                        {aov->normal, 12u * n},
                        {aov->depth, 4u * n},
                        {aov->hits, 4u * n},
                        {edges ? aov->object : nullptr, 4u * n}};
  return check_overlap(outs, ins, -1, -1, "an output overlaps an input", "two outputs overlap");
}

/* the launch of a checked call, on the current device */
int upsample_launch(const float *low_rgb, const RtHipAov *low_aov, int32_t low_width, int32_t low_height, const RtHipAov *aov,
                    int32_t width, int32_t height, const RtHipUpsampleParams *p, float *out_rgb, uint8_t *out_rgb8, float *out_conf,
                    hipStream_t stream)
{
  PtUpsample U = {};
  U.demodulate = (p->flags & RT_HIP_UPSAMPLE_DEMODULATE) ? 1u : 0u;
  U.object_edges = (p->flags & RT_HIP_UPSAMPLE_OBJECT_EDGES) ? 1u : 0u;
  U.low_rgb = low_rgb;
  U.low_albedo = U.demodulate ? low_aov->albedo : nullptr;
  U.low_normal = low_aov->normal;
  U.low_depth = low_aov->depth;
  U.low_hits = low_aov->hits;
  U.low_object = U.object_edges ? low_aov->object : nullptr;
  U.albedo = U.demodulate ? aov->albedo : nullptr;
  U.normal = aov->normal;
  U.depth = aov->depth;
  U.hits = aov->hits;
  U.object = U.object_edges ? aov->object : nullptr;
  U.out_rgb = out_rgb;
  U.out_rgb8 = out_rgb8;
  U.out_conf = out_conf;
  U.low_width = low_width;
  U.low_height = low_height;
  U.width = width;
  U.height = height;
  U.normal_power_log2 = p->normal_power_log2;
  U.sigma_depth = p->sigma_depth;
  return launched(pt_launch_upsample(U, stream), "pt_upsample");
}

int upsample_image_impl(const float *h_low_rgb, const RtHipAov *h_low_aov, int32_t low_width, int32_t low_height, const RtHipAov *h_aov,
                        int32_t width, int32_t height, const RtHipUpsampleParams *params, int device, float *h_out_rgb,
                        uint8_t *h_out_rgb8, float *h_out_conf)
{
  if (const int rc = check_upsample(h_low_rgb, h_low_aov, low_width, low_height, h_aov, width, height, params, h_out_rgb, h_out_rgb8, h_out_conf))
    return rc;
  return on_logical_device(device, [&](int) {
    const bool demod = (params->flags & RT_HIP_UPSAMPLE_DEMODULATE) != 0u, edges = (params->flags & RT_HIP_UPSAMPLE_OBJECT_EDGES) != 0u;
    const size_t nl = (size_t)low_width * (size_t)low_height, n = (size_t)width * (size_t)height;
    /* per frame -- low, then full -- the buffers the flags ask for; then the low colour, the result, the confidence, the bytes */
    StageArena A;
    const AovStage low_aov(A, h_low_aov, nl, demod, edges), aov(A, h_aov, n, demod, edges);
    const int low_rgb = A.part(12u * nl, h_low_rgb);
    const int out = A.part(12u * n, nullptr, h_out_rgb);
    const int conf = A.part(4u * n, nullptr, h_out_conf, h_out_conf != nullptr);
    const int rgb8 = A.part(3u * n, nullptr, h_out_rgb8, h_out_rgb8 != nullptr);
    int rc = A.stage();
    if (rc)
      return rc;
    const RtHipAov d_low_aov = low_aov.device(A), d_aov = aov.device(A);
    rc = upsample_launch(A.at<float>(low_rgb), &d_low_aov, low_width, low_height, &d_aov, width, height, params, A.at<float>(out),
                         A.at<uint8_t>(rgb8), A.at<float>(conf), nullptr);
    return rc ? rc : A.download();
  });
}

/* ---- ray queries (rt_hip.h, rt_hip_query_*) ---------------------------------------------------------------------------------
 * A query's launch takes the scene- and near_R-dependent fields of launch_prepare with origin_radius in the camera distance's
 * place, and acquire_tables' filter, hierarchy and fp32 triangle table for that near_R -- what intersect() reads -- and nothing
 * else: no plan, no pool, no status word (as an AOV launch).  The walls are not pruned among themselves (big_pairs stays 0). */
bool hits_any(const RtHipHits *h)
{
  return h && (h->status || h->t || h->object || h->prim || h->point || h->normal || h->bary || h->ray);
}

/* the ray front end's arguments (a ray query's and a radiance query's alike) that need no device: RT_HIP_EINVAL, or RT_HIP_OK */
int check_rays(const void *rays, bool device_rays, uint64_t n, uint32_t source, uint32_t flags, const RtHipCamera *camera, double origin_radius)
{
  if (n > 0xFFFFFFFFull)
    return fail(RT_HIP_EINVAL, "n = %llu: a query takes fewer than 2^32 rays", (unsigned long long)n);
  if (source != RT_HIP_RAYS_GIVEN && source != RT_HIP_RAYS_CAMERA_UV)
    return fail(RT_HIP_EINVAL, "source %u is neither RT_HIP_RAYS_GIVEN nor RT_HIP_RAYS_CAMERA_UV", source);
  if (flags & ~(uint32_t)RT_HIP_RAYS_NORMALIZE)
    return fail(RT_HIP_EINVAL, "unknown flags %#x", flags);
  if (!(origin_radius >= 0) || !std::isfinite(origin_radius))
    return fail(RT_HIP_EINVAL, "origin_radius %g must be finite and >= 0", origin_radius);
  if (source == RT_HIP_RAYS_CAMERA_UV && !camera)
    return fail(RT_HIP_EINVAL, "RT_HIP_RAYS_CAMERA_UV needs params->camera");
  if (n != 0 && !rays)
    return fail(RT_HIP_EINVAL, "rays is required");
  if (device_rays && (reinterpret_cast<uintptr_t>(rays) & 15u))
    return fail(RT_HIP_EINVAL, "d_rays must be 16-byte aligned");
  return RT_HIP_OK;
}

/* the arguments of a query that need no device: RT_HIP_EINVAL, or RT_HIP_OK */
int check_query(const void *rays, bool device_rays, uint64_t n, const RtHipQueryParams *p, const RtHipHits *hits)
{
  if (!p)
    return fail(RT_HIP_EINVAL, "params is required");
  if (!hits_any(hits))
    return fail(RT_HIP_EINVAL, "hits: at least one output array is required");
  return check_rays(rays, device_rays, n, p->source, p->flags, p->camera, p->origin_radius);
}

/* The launch of a kernel that scans for rays of the caller's (a ray query, a radiance query): the scene- and near_R-dependent
 * fields of launch_prepare with origin_radius in the camera distance's place, the camera of RT_HIP_RAYS_CAMERA_UV, and nothing a
 * rule of the renderer's own rays needs -- the walls are not pruned among themselves (big_pairs stays 0) and no ray leaves a hull
 * facet (the rule is the parked walks').  L is cleared first. */
int ray_launch_prepare(const RtHipScene *scene, uint32_t source, const RtHipCamera *camera, double origin_radius, PtLaunch &L)
{
  memset(&L, 0, sizeof L);
  L.scene = scene->view;
  if (source == RT_HIP_RAYS_CAMERA_UV)
    camera_of(camera, L.cam);
  L.near_R = 1.5 * (origin_radius + scene->reach) + 1.0;
  if (!(L.near_R < RT_NEAR_R_LIMIT))
    return fail(RT_HIP_EINVAL, "origin_radius and scene extent give near_R = %g: not a usable finite bound", L.near_R);
  L.near_R2 = L.near_R * L.near_R;
  L.filt_shift = 12.0 * 5.9604644775390625e-08 * (scene->max_center + L.near_R) * (1.0 + 1e-9);
  mesh_bound_for(scene, L.near_R, L.mesh_bound);
  L.hull_margin = 2.0;
  L.background = 10 / 255.0;
  L.t_start = 1.7976931348623157e308; /* DBL_MAX */
  return RT_HIP_OK;
}

/* One launch of a kernel that reads a scene's camera-dependent tables (an AOV, a query, a radiance query, a pixel refinement): the
 * scene's device made current, the tables for L.near_R acquired on `stream`, `launch` (-> hipError_t) run, the tables released, a
 * failure named after the kernel */
template <class Launch>
int launch_with_tables(const RtHipScene *scene, PtLaunch &L, hipStream_t stream, const char *kernel, Launch launch)
{
  DeviceScope scope(scene->device);
  HIP_TRY(scope.status);
  size_t slot = 0;
  const int rc = acquire_tables(scene, L.near_R, stream, &L.scene.filt, &L.scene.bvh_nodes, &slot);
  if (rc)
    return rc;
  const hipError_t e = launch();
  release_tables(scene, slot, stream);
  return launched(e, kernel);
}

int query_launch(const RtHipScene *scene, const double *d_rays, const double *d_t_max, uint64_t n, const RtHipQueryParams *p,
                 const RtHipHits *d_hits, hipStream_t stream)
{
  PtLaunch L;
  const int rc = ray_launch_prepare(scene, p->source, p->camera, p->origin_radius, L);
  if (rc)
    return rc;
  const PtQuery Q = {.rays = d_rays, .t_max = d_t_max, .n = n, .camera_uv = p->source == RT_HIP_RAYS_CAMERA_UV ? 1u : 0u,
                     .normalize = (p->flags & RT_HIP_RAYS_NORMALIZE) ? 1u : 0u, .status = d_hits->status, .t = d_hits->t,
                     .object = d_hits->object, .prim = d_hits->prim, .point = d_hits->point, .normal = d_hits->normal,
                     .bary = d_hits->bary, .ray = d_hits->ray};
  const int which = pt_query_pick(scene->view);
  return launch_with_tables(scene, L, stream, pt_query_kernel_name_of(which), [&] { return pt_launch_query(L, Q, stream, which); });
}

/* rt_hip_query_rays_host: a scene of its own on the logical device, one allocation for the rays, the limits and the requested
 * outputs, the query on the null stream, the copies.  Everything is owned by this scope. */
int query_rays_host_impl(const RtHipSphere *spheres, size_t n_spheres, const RtHipMesh *meshes, size_t n_meshes, const double *h_rays,
                         const double *h_t_max, uint64_t n, const RtHipQueryParams *params, int device, const RtHipHits *h_hits)
{
  int rc = check_query(h_rays, false, n, params, h_hits);
  if (rc)
    return rc;
  if (n == 0)
  { /* (the device is looked up before an empty query returns) */
    int phys = -1;
    return physical_device(device, &phys);
  }
  return with_owned_scene(spheres, n_spheres, meshes, n_meshes, device, [&](const RtHipScene *scene, int) {
    void *host[8] = {h_hits->status, h_hits->t, h_hits->object, h_hits->prim, h_hits->point, h_hits->normal, h_hits->bary, h_hits->ray};
    const size_t bytes_per_ray[8] = {4, 8, 4, 4, 24, 24, 16, 48};
    StageArena A;
    const int rays = A.part((params->source == RT_HIP_RAYS_CAMERA_UV ? 16u : 48u) * n, h_rays);
    const int t_max = A.part(8u * n, h_t_max, nullptr, h_t_max != nullptr);
    int out[8];
    for (int k = 0; k < 8; k++)
      out[k] = A.part(bytes_per_ray[k] * n, nullptr, host[k], host[k] != nullptr);
    rc = A.stage();
    if (rc)
      return rc;
    const RtHipHits d_hits = {A.at<uint32_t>(out[0]), A.at<double>(out[1]), A.at<uint32_t>(out[2]), A.at<uint32_t>(out[3]),
                              A.at<double>(out[4]),   A.at<double>(out[5]), A.at<double>(out[6]),   A.at<double>(out[7])};
    rc = query_launch(scene, A.at<double>(rays), A.at<double>(t_max), n, params, &d_hits, nullptr);
    return rc ? rc : A.download();
  });
}

/* ---- radiance queries (rt_hip.h, rt_hip_trace_*) ------------------------------------------------------------------------------
 * A radiance query's launch is a query's launch (origin_radius in the camera distance's place, acquire_tables) that traces paths:
 * it also takes what a render launch of a static M_REFRACTION member takes -- samples, max_depth and seed, the device's status word
 * (status_word_for) and a slot pool of pending-ray stacks (pend_pool_for under g_pend_mutex, from the lookup until the launch is
 * enqueued, as rt_hip_render_tiles_chunked holds it).  No plan: the scene alone picks the form, and every form is a PEND_POOL kernel
 * of PT_PEND_COLUMNS stacks per slot.  BigPrune and the hull-facet rule stay off (big_pairs 0, margin 2), as for a query. */
bool radiance_any(const RtHipRadiance *o)
{
  return o && (o->status || o->radiance || o->samples || o->paths || o->casts || o->ray);
}

/* What every form that traces paths refuses in its integrator, samples and max_depth, in that order; `what` names the form.  A
 * form that checks something else between them (a pixel refinement, a bake) calls the parts. */
int check_integrator(uint32_t integrator, const char *what)
{
  if (integrator != RT_HIP_TRACE_PATH)
    return fail(RT_HIP_EINVAL, "integrator %u: %s traces paths (RT_HIP_TRACE_PATH) only", integrator, what);
  return RT_HIP_OK;
}

int check_max_depth(int32_t max_depth)
{
  if (max_depth < 0 || max_depth > 1000000)
    return fail(RT_HIP_EINVAL, "max_depth out of range");
  return RT_HIP_OK;
}

int check_path_fields(uint32_t integrator, int32_t samples, int32_t max_depth, const char *what)
{
  if (const int rc = check_integrator(integrator, what))
    return rc;
  if (samples < 1)
    return fail(RT_HIP_EINVAL, "samples = %d must be >= 1", samples);
  return check_max_depth(max_depth);
}

/* the arguments of a radiance query that need no device: RT_HIP_EINVAL, or RT_HIP_OK */
int check_trace(const void *rays, bool device_rays, uint64_t n, const RtHipTraceParams *p, const RtHipRadiance *out)
{
  if (!p)
    return fail(RT_HIP_EINVAL, "params is required");
  if (!radiance_any(out))
    return fail(RT_HIP_EINVAL, "radiance: at least one output array is required");
  if (const int rc = check_path_fields(p->integrator, p->samples, p->max_depth, "a radiance query"))
    return rc;
  if (n > 0xFFFFFFFFull || (uint64_t)p->index_first + n > 0x100000000ull)
    return fail(RT_HIP_EINVAL, "n = %llu, index_first = %u: a radiance query takes fewer than 2^32 rays with stream indices below 2^32",
                (unsigned long long)n, p->index_first);
  return check_rays(rays, device_rays, n, p->source, p->flags, p->camera, p->origin_radius);
}

/* What a radiance query's and a pixel refinement's launch start from: the depth limit of the fixed pending-ray stack, a query's
 * launch (ray_launch_prepare), and the path tracer's own fields */
int pooled_launch_prepare(const RtHipScene *scene, uint32_t source, const RtHipCamera *camera, double origin_radius, int32_t samples,
                          int32_t max_depth, uint64_t seed, uint64_t *d_stats, PtLaunch &L)
{
  if (scene->view.any_refract && max_depth > PT_REFRACT_MAX_DEPTH)
    return fail(RT_HIP_ELIMIT, "scenes with M_REFRACTION materials support max_depth <= %d (two rays per refractive hit, "
                               "raytracer.c:523-529; the pending-ray stack is fixed)", PT_REFRACT_MAX_DEPTH);
  const int rc = ray_launch_prepare(scene, source, camera, origin_radius, L);
  if (rc)
    return rc;
  L.samples = samples;
  L.max_depth = max_depth;
  L.seed = seed;
  L.stats = reinterpret_cast<unsigned long long *>(d_stats);
  return RT_HIP_OK;
}

/* ... and how they are launched: launch_with_tables with the device's status word, and its slot pool of pending-ray stacks held
 * under g_pend_mutex from the lookup until `launch` has enqueued the kernel */
template <class Launch>
int pooled_launch(const RtHipScene *scene, PtLaunch &L, hipStream_t stream, const char *kernel, Launch launch)
{
  DeviceScope scope(scene->device);
  HIP_TRY(scope.status);
  int rc = status_word_for(scene->device, &L.status);
  if (rc)
    return rc;
  int pool_rc = RT_HIP_OK;
  rc = launch_with_tables(scene, L, stream, kernel, [&] {
    std::lock_guard<std::mutex> pend_lock(g_pend_mutex);
    pool_rc = pend_pool_for(scene->device, pt_pend_entries(scene->view, 0u, L.max_depth), PT_PEND_COLUMNS, L);
    return pool_rc ? hipSuccess : launch();
  });
  return pool_rc ? pool_rc : rc;
}

int trace_launch(const RtHipScene *scene, const double *d_rays, uint64_t n, const RtHipTraceParams *p, const RtHipRadiance *d_out,
                 uint64_t *d_stats, hipStream_t stream)
{
  PtLaunch L;
  const int rc = pooled_launch_prepare(scene, p->source, p->camera, p->origin_radius, p->samples, p->max_depth, p->seed, d_stats, L);
  if (rc)
    return rc;
  const PtTrace T = {.rays = d_rays, .n = n, .camera_uv = p->source == RT_HIP_RAYS_CAMERA_UV ? 1u : 0u,
                     .normalize = (p->flags & RT_HIP_RAYS_NORMALIZE) ? 1u : 0u, .index_first = p->index_first, .status = d_out->status,
                     .radiance = d_out->radiance, .samples = d_out->samples, .paths = reinterpret_cast<unsigned long long *>(d_out->paths),
                     .casts = reinterpret_cast<unsigned long long *>(d_out->casts), .ray = d_out->ray};
  const int which = pt_trace_pick(scene->view);
  return pooled_launch(scene, L, stream, pt_trace_kernel_name_of(which), [&] { return pt_launch_trace(L, T, stream, which); });
}

/* rt_hip_trace_rays_host: a scene of its own on the logical device, one allocation for the rays, the counters and the requested
 * outputs, the launch on the null stream, the copies.  Everything is owned by this scope. */
int trace_rays_host_impl(const RtHipSphere *spheres, size_t n_spheres, const RtHipMesh *meshes, size_t n_meshes, const double *h_rays,
                         uint64_t n, const RtHipTraceParams *params, int device, const RtHipRadiance *h_out, uint64_t *h_stats)
{
  int rc = check_trace(h_rays, false, n, params, h_out);
  if (rc || n == 0)
    return rc; /* (no ray: nothing to do, on any device or none) */
  return with_owned_scene(spheres, n_spheres, meshes, n_meshes, device, [&](const RtHipScene *scene, int) {
    StageArena A;
    const int rays = A.part((params->source == RT_HIP_RAYS_CAMERA_UV ? 16u : 48u) * n, h_rays);
    RadianceStage R(A, h_out, n, params->samples, h_stats);
    rc = A.stage();
    if (rc)
      return rc;
    const RtHipRadiance d_out = R.device(A);
    rc = trace_launch(scene, A.at<double>(rays), n, params, &d_out, A.at<uint64_t>(R.stats), nullptr);
    return rc ? rc : R.download(A);
  });
}

/* ---- generated-ray jobs: what a lens frame and a probe bake share ---------------------------------------------------------------
 * A job is `total` ray indices cut into slices of at most `slice`, a slice ending at every multiple of `period` as well.  Per slice,
 * on one stream and with no host wait: the caller's generator writes the rays of indices [first, first + n), the radiance query as it
 * stands (trace_launch, one sample a ray, index_first = first) traces them, the caller's fold adds them into the job's sums; after the
 * last slice the caller's resolve.  The workspace: a slice's rays, status words and radiance, then sum_bytes of sums. */
struct SliceWorkspace
{
  size_t rays, status, radiance, sum, total;
  SliceWorkspace(uint64_t slice, size_t sum_bytes)
  {
    rays = 0;
    status = rays + stage_align(48u * slice);
    radiance = status + stage_align(4u * slice);
    sum = radiance + stage_align(24u * slice);
    total = sum + stage_align(sum_bytes);
  }
};

/* ... as pointers: the sums are the caller's d_sum where it gives one */
struct SliceBuffers
{
  double *rays;
  uint32_t *status;
  double *radiance, *sum;
};

struct SlicedJob
{
  double origin_radius; /* trace_launch's, with max_depth and seed */
  int32_t max_depth;
  uint64_t seed;
  uint64_t total, slice, period;
  size_t sum_bytes;
  void *d_workspace;
  double *d_sum;
  uint64_t *d_stats;
};

/* The job on `stream`: trace_launch's own refusals (the depth limit, near_R) asked for once, up front; then, with the scene's device
 * current, the sums cleared, write(B, first, n) and fold(B, first, n) around every slice's trace_launch, and resolve(B).  Each
 * callable -> RT_HIP_*. */
template <class Write, class Fold, class Resolve>
int sliced_trace(const RtHipScene *scene, const SlicedJob &J, hipStream_t stream, Write write, Fold fold, Resolve resolve)
{
  RtHipTraceParams T;
  rt_hip_trace_defaults(&T);
  T.origin_radius = J.origin_radius;
  T.samples = 1;
  T.max_depth = J.max_depth;
  T.seed = J.seed;
  {
    PtLaunch dry;
    const int rc = pooled_launch_prepare(scene, T.source, nullptr, T.origin_radius, 1, T.max_depth, T.seed, nullptr, dry);
    if (rc)
      return rc;
  }
  DeviceScope scope(scene->device);
  HIP_TRY(scope.status);
  const SliceWorkspace W(J.slice, J.sum_bytes);
  char *const ws = static_cast<char *>(J.d_workspace);
  const SliceBuffers B = {reinterpret_cast<double *>(ws + W.rays), reinterpret_cast<uint32_t *>(ws + W.status),
                          reinterpret_cast<double *>(ws + W.radiance), J.d_sum ? J.d_sum : reinterpret_cast<double *>(ws + W.sum)};
  HIP_TRY(hipMemsetAsync(B.sum, 0, J.sum_bytes, stream));
  const RtHipRadiance out = {B.status, B.radiance, nullptr, nullptr, nullptr, nullptr};
  for (uint64_t first = 0, n; first < J.total; first += n)
  {
    n = std::min<uint64_t>(J.slice, J.period - first % J.period);
    int rc = write(B, first, (uint32_t)n);
    if (rc)
      return rc;
    T.index_first = (uint32_t)first;
    rc = trace_launch(scene, B.rays, n, &T, &out, J.d_stats, stream);
    if (rc)
      return rc;
    rc = fold(B, first, (uint32_t)n);
    if (rc)
      return rc;
  }
  return resolve(B);
}

/* rt_hip_render_lens' and rt_hip_bake_probes' rule for the job's buffers (null pointers pass: each call has its own text for them) */
int check_slice_buffers(const void *d_workspace, const double *d_sum)
{
  if (reinterpret_cast<uintptr_t>(d_workspace) & 15u) /* (the slice's rays lie at its start: rt_hip_trace_rays' own rule) */
    return fail(RT_HIP_EINVAL, "d_workspace must be 16-byte aligned");
  if (reinterpret_cast<uintptr_t>(d_sum) & 7u)
    return fail(RT_HIP_EINVAL, "d_sum must be 8-byte aligned");
  return RT_HIP_OK;
}

/* the slice of the host forms, in rays a launch: 160 MB of rays, status words and radiance at most */
constexpr uint32_t HOST_SLICE = 1u << 21;

/* ... and their end: the copies, then the device's status word as the call's answer */
int download_then_status(const StageArena &A, int phys)
{
  if (const int rc = A.download())
    return rc;
  uint32_t flags = 0;
  const int rc = status_take(phys, &flags);
  return rc ? rc : status_to_error(flags);
}

/* ---- thin-lens camera (rt_hip.h, rt_hip_lens_* / rt_hip_render_lens*) ---------------------------------------------------------
 * A lens frame is a generated-ray job (above): lens rays (lens.hip), a per-pixel sum (lens.hip), one sample pass of the frame a
 * period.  The checks need no device; the frame refuses everything it can before its first launch. */
int check_lens(const RtHipCamera *camera, const RtHipLens *lens, int32_t width, int32_t height)
{
  if (!camera || !lens)
    return fail(RT_HIP_EINVAL, "camera and lens are required");
  if (!(lens->aperture_radius >= 0) || !std::isfinite(lens->aperture_radius))
    return fail(RT_HIP_EINVAL, "aperture_radius %g must be finite and >= 0", lens->aperture_radius);
  if (!(lens->focus_distance > 0) || !std::isfinite(lens->focus_distance))
    return fail(RT_HIP_EINVAL, "focus_distance %g must be finite and > 0", lens->focus_distance);
  if (lens->flags != 0u || lens->reserved != 0u)
    return fail(RT_HIP_EINVAL, "lens flags and reserved must be 0");
  if (!frame_size_ok(width, height, 2))
    return fail(RT_HIP_EINVAL, "width and height must be in [2, 2^20] with fewer than 2^32 pixels");
  return RT_HIP_OK;
}

/* vec3_normalize (vector.h:53-58) on the host: v * (1.0 / sqrt((x*x + y*y) + z*z)) */
void lens_axis(const double v[3], double out[3])
{
  const double inv = 1.0 / std::sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
  for (int k = 0; k < 3; k++)
    out[k] = v[k] * inv;
}

/* the generator's arguments but for the range (pixel_first, n, index_first) and the output */
PtLensRays lens_args(const RtHipCamera *camera, const RtHipLens *lens, int32_t width, int32_t height, uint64_t seed)
{
  PtLensRays A;
  memset(&A, 0, sizeof A);
  memcpy(A.position, camera->position, sizeof A.position);
  memcpy(A.horizontal, camera->horizontal, sizeof A.horizontal);
  memcpy(A.vertical, camera->vertical, sizeof A.vertical);
  memcpy(A.lower_left_corner, camera->lower_left_corner, sizeof A.lower_left_corner);
  lens_axis(camera->horizontal, A.ax);
  lens_axis(camera->vertical, A.ay);
  A.w_minus_1 = (double)width - 1.0;
  A.h_minus_1 = (double)height - 1.0;
  A.aperture_radius = lens->aperture_radius;
  A.focus_distance = lens->focus_distance;
  A.seed = seed;
  A.lens_seed = rt_mix64(seed ^ 0x6C656E73ull);
  A.width = (uint32_t)width;
  return A;
}

/* a lens frame's workspace: slices never exceed the frame, the sums are three doubles a pixel */
SliceWorkspace lens_workspace(uint64_t n_pixels, uint64_t slice_pixels)
{
  return SliceWorkspace(std::min<uint64_t>(slice_pixels, n_pixels), 24u * n_pixels);
}

/* what rt_hip_render_lens refuses without a device: RT_HIP_EINVAL, or RT_HIP_OK */
int check_render_lens(const RtHipCamera *camera, const RtHipLens *lens, const RtHipParams *p, uint32_t slice_pixels, bool any_output)
{
  if (!p)
    return fail(RT_HIP_EINVAL, "params is required");
  if (const int rc = check_lens(camera, lens, p->width, p->height))
    return rc;
  if (!any_output)
    return fail(RT_HIP_EINVAL, "at least one of sum, rgb and rgb8 is required");
  if (const int rc = check_path_fields(p->integrator, p->samples, p->max_depth, "a lens frame"))
    return rc;
  const uint64_t n_pixels = (uint64_t)p->width * (uint64_t)p->height;
  if ((uint64_t)p->samples * n_pixels > 0x100000000ull)
    return fail(RT_HIP_EINVAL, "samples x pixels = %d x %llu exceeds 2^32: a lens sample is a ray index of rt_hip_trace_rays", p->samples,
                (unsigned long long)n_pixels);
  if (slice_pixels == 0u)
    return fail(RT_HIP_EINVAL, "slice_pixels must be >= 1");
  const uint64_t n_tiles = (uint64_t)tiles_x_of(p->width) * tiles_y_of(p->height);
  if (p->tile_first != 0u || p->tile_stride > 1u || (p->tile_count != 0u && p->tile_count != n_tiles))
    return fail(RT_HIP_EINVAL, "a lens frame is the whole frame: the tile fields must describe it or be 0");
  return RT_HIP_OK;
}

/* The frame: a job of samples x pixels ray indices, a sample pass a period -- so pixel_first = first % pixels and no slice spans two
 * passes --, then the resolve.  All on `stream`, no host wait. */
int render_lens_launch(const RtHipScene *scene, const RtHipCamera *camera, const RtHipLens *lens, const RtHipParams *p, uint32_t slice_pixels,
                       void *d_workspace, double *d_sum, float *d_rgb, uint8_t *d_rgb8, uint64_t *d_stats, hipStream_t stream)
{
  const uint64_t n_pixels = (uint64_t)p->width * (uint64_t)p->height;
  const double origin_radius = std::sqrt((camera->position[0] * camera->position[0] + camera->position[1] * camera->position[1]) +
                                         camera->position[2] * camera->position[2]) + lens->aperture_radius;
  if (!std::isfinite(origin_radius))
    return fail(RT_HIP_EINVAL, "the camera position is not finite");
  const SlicedJob J = {.origin_radius = origin_radius, .max_depth = p->max_depth, .seed = p->seed, .total = (uint64_t)p->samples * n_pixels,
                       .slice = std::min<uint64_t>(slice_pixels, n_pixels), .period = n_pixels, .sum_bytes = 24u * n_pixels,
                       .d_workspace = d_workspace, .d_sum = d_sum, .d_stats = d_stats};
  PtLensRays A = lens_args(camera, lens, p->width, p->height, p->seed);
  return sliced_trace(
      scene, J, stream,
      [&](const SliceBuffers &B, uint64_t first, uint32_t n) {
        A.rays = B.rays;
        A.pixel_first = (uint32_t)(first % n_pixels);
        A.n = n;
        A.index_first = (uint32_t)first;
        return launched(lens_launch_rays(A, stream), "k_lens_rays");
      },
      [&](const SliceBuffers &B, uint64_t first, uint32_t n) {
        return launched(lens_launch_accumulate(B.status, B.radiance, (uint32_t)(first % n_pixels), n, B.sum, stream), "k_lens_accumulate");
      },
      [&](const SliceBuffers &B) {
        return d_rgb || d_rgb8 ? launched(lens_launch_resolve(B.sum, n_pixels, p->samples, d_rgb, d_rgb8, stream), "k_lens_resolve") : (int)RT_HIP_OK;
      });
}

/* rt_hip_render_lens_image: a scene of its own on the logical device, one allocation for the workspace, the frame and the counters,
 * the frame on the null stream, the copies, the device's status word.  Everything is owned by this scope. */
int render_lens_image_impl(const RtHipSphere *spheres, size_t n_spheres, const RtHipMesh *meshes, size_t n_meshes, const RtHipCamera *camera,
                           const RtHipLens *lens, const RtHipParams *params, int device, float *h_rgb, uint8_t *h_rgb8, uint64_t *h_stats)
{
  if (const int rc = check_render_lens(camera, lens, params, HOST_SLICE, h_rgb || h_rgb8))
    return rc;
  return with_owned_scene(spheres, n_spheres, meshes, n_meshes, device, [&](const RtHipScene *scene, int phys) {
    const uint64_t n_pixels = (uint64_t)params->width * (uint64_t)params->height;
    StageArena A;
    const int ws = A.part(lens_workspace(n_pixels, HOST_SLICE).total);
    const int rgb = A.part(12u * n_pixels, nullptr, h_rgb, h_rgb != nullptr);
    const int rgb8 = A.part(3u * n_pixels, nullptr, h_rgb8, h_rgb8 != nullptr);
    const int stats = A.zeroed(RT_HIP_NSTATS * sizeof(uint64_t), h_stats);
    int rc = A.stage();
    if (rc)
      return rc;
    rc = render_lens_launch(scene, camera, lens, params, HOST_SLICE, A.at<char>(ws), nullptr, A.at<float>(rgb), A.at<uint8_t>(rgb8),
                            A.at<uint64_t>(stats), nullptr);
    return rc ? rc : download_then_status(A, phys);
  });
}

/* ---- light probes (rt_hip.h, rt_hip_probe_* / rt_hip_bake_probes*) -------------------------------------------------------------
 * A bake is a generated-ray job (above): probe rays (probe.hip), a per-probe fold (probe.hip), the whole bake one period.  The checks
 * need no device; the bake refuses everything it can before its first launch. */
uint32_t probe_bases(uint32_t mode) { return mode == RT_HIP_PROBE_HEMISPHERE ? 1u : (uint32_t)PT_PROBE_SH; }

/* what every probe call refuses in its params without a device: RT_HIP_EINVAL, or RT_HIP_OK */
int check_probe(const RtHipProbeParams *p, uint64_t n_probes, bool have_normals)
{
  if (!p)
    return fail(RT_HIP_EINVAL, "params is required");
  if (p->mode != RT_HIP_PROBE_SPHERE && p->mode != RT_HIP_PROBE_HEMISPHERE)
    return fail(RT_HIP_EINVAL, "mode %u is neither RT_HIP_PROBE_SPHERE nor RT_HIP_PROBE_HEMISPHERE", p->mode);
  if (p->flags != 0u || p->reserved != 0u)
    return fail(RT_HIP_EINVAL, "probe flags and reserved must be 0");
  if (p->samples < 1)
    return fail(RT_HIP_EINVAL, "samples = %d must be >= 1", p->samples);
  if (n_probes > 0x100000000ull || n_probes * (uint64_t)p->samples > 0x100000000ull)
    return fail(RT_HIP_EINVAL, "probes x samples = %llu x %d exceeds 2^32: a probe sample is a ray index of rt_hip_trace_rays",
                (unsigned long long)n_probes, p->samples);
  if (!(p->bias >= 0) || !std::isfinite(p->bias))
    return fail(RT_HIP_EINVAL, "bias %g must be finite and >= 0", p->bias);
  if (!(p->origin_radius >= 0) || !std::isfinite(p->origin_radius))
    return fail(RT_HIP_EINVAL, "origin_radius %g must be finite and >= 0", p->origin_radius);
  if (const int rc = check_max_depth(p->max_depth))
    return rc;
  if (p->mode == RT_HIP_PROBE_HEMISPHERE && !have_normals && n_probes != 0)
    return fail(RT_HIP_EINVAL, "RT_HIP_PROBE_HEMISPHERE needs normals");
  return RT_HIP_OK;
}

/* the generator's arguments but for the range (k_first, n) and the output */
PtProbeRays probe_args(const double *d_positions, const double *d_normals, const RtHipProbeParams *p)
{
  PtProbeRays A;
  memset(&A, 0, sizeof A);
  A.positions = d_positions;
  A.normals = d_normals;
  A.probe_seed = rt_mix64(p->seed ^ PT_PROBE_KEY);
  A.bias = p->bias;
  A.samples = (uint32_t)p->samples;
  A.hemisphere = p->mode == RT_HIP_PROBE_HEMISPHERE ? 1u : 0u;
  return A;
}

/* a bake's workspace: the sums are three doubles a basis and probe */
SliceWorkspace probe_workspace(uint64_t n_probes, uint32_t mode, uint64_t slice_rays)
{
  return SliceWorkspace(slice_rays, 24u * probe_bases(mode) * n_probes);
}

int probe_resolve_launch(const double *d_sum, uint64_t n_probes, uint32_t mode, int32_t samples, double *d_coeff, float *d_coeff_f,
                         hipStream_t stream)
{
  const double k = mode == RT_HIP_PROBE_HEMISPHERE ? PT_PROBE_K_HEMISPHERE : PT_PROBE_K_SPHERE;
  return launched(probe_launch_resolve(d_sum, 3u * probe_bases(mode) * n_probes, samples, k, d_coeff, d_coeff_f, stream), "k_probe_resolve");
}

/* The bake: a job of probes x samples ray indices in one period, the probes' status words marked before the first slice's rays are
 * written, then the resolve.  All on `stream`, no host wait.  n_probes >= 1. */
int bake_probes_launch(const RtHipScene *scene, const double *d_positions, const double *d_normals, uint64_t n_probes,
                       const RtHipProbeParams *p, uint32_t slice_rays, void *d_workspace, double *d_sum, double *d_coeff, float *d_coeff_f,
                       uint32_t *d_status, uint64_t *d_stats, hipStream_t stream)
{
  const uint64_t total = n_probes * (uint64_t)p->samples, S = (uint64_t)p->samples;
  const SlicedJob J = {.origin_radius = p->origin_radius, .max_depth = p->max_depth, .seed = p->seed, .total = total,
                       .slice = std::min<uint64_t>(slice_rays, total), .period = total, .sum_bytes = 24u * probe_bases(p->mode) * n_probes,
                       .d_workspace = d_workspace, .d_sum = d_sum, .d_stats = d_stats};
  PtProbeRays A = probe_args(d_positions, d_normals, p);
  PtProbeFold F;
  memset(&F, 0, sizeof F);
  F.normals = d_normals;
  F.probe_status = d_status;
  F.samples = A.samples;
  F.hemisphere = A.hemisphere;
  return sliced_trace(
      scene, J, stream,
      [&](const SliceBuffers &B, uint64_t first, uint32_t n) {
        if (first == 0 && d_status)
          HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(d_status), 1, n_probes, stream));
        A.rays = B.rays;
        A.k_first = first;
        A.n = n;
        return launched(probe_launch_rays(A, stream), "k_probe_rays");
      },
      [&](const SliceBuffers &B, uint64_t first, uint32_t n) {
        F.rays = B.rays;
        F.radiance = B.radiance;
        F.status = B.status;
        F.sum = B.sum;
        F.k_first = first;
        F.n = n;
        F.probe_first = first / S;
        F.n_probes = (first + n - 1u) / S - F.probe_first + 1u;
        return launched(probe_launch_fold(F, stream), "k_probe_fold");
      },
      [&](const SliceBuffers &B) { /* (no d_coeff: an update round's job, which stops at its sums) */
        return d_coeff ? probe_resolve_launch(B.sum, n_probes, p->mode, p->samples, d_coeff, d_coeff_f, stream) : (int)RT_HIP_OK;
      });
}

/* rt_hip_bake_probes_host: a scene of its own on the logical device, one allocation for the probes, the workspace, the outputs and
 * the counters, the bake on the null stream, the copies, the device's status word.  Everything is owned by this scope. */
int bake_probes_host_impl(const RtHipSphere *spheres, size_t n_spheres, const RtHipMesh *meshes, size_t n_meshes, const double *h_positions,
                          const double *h_normals, uint64_t n_probes, const RtHipProbeParams *params, int device, double *h_coeff,
                          float *h_coeff_f, uint32_t *h_status, uint64_t *h_stats)
{
  int rc = check_probe(params, n_probes, h_normals != nullptr);
  if (rc || n_probes == 0)
    return rc; /* (no probe: nothing to do, on any device or none) */
  if (!h_positions || !h_coeff)
    return fail(RT_HIP_EINVAL, "h_positions and h_coeff are required");
  return with_owned_scene(spheres, n_spheres, meshes, n_meshes, device, [&](const RtHipScene *scene, int phys) {
    const bool hemisphere = params->mode == RT_HIP_PROBE_HEMISPHERE;
    const uint32_t bases = probe_bases(params->mode);
    const uint64_t total = n_probes * (uint64_t)params->samples;
    StageArena A;
    const int ws = A.part(probe_workspace(n_probes, params->mode, std::min<uint64_t>(HOST_SLICE, total)).total);
    const int positions = A.part(24u * n_probes, h_positions);
    const int normals = A.part(24u * n_probes, h_normals, nullptr, hemisphere);
    const int coeff = A.part(24u * bases * n_probes, nullptr, h_coeff);
    const int coeff_f = A.part(12u * bases * n_probes, nullptr, h_coeff_f, h_coeff_f != nullptr);
    const int status = A.part(4u * n_probes, nullptr, h_status, h_status != nullptr);
    const int stats = A.zeroed(RT_HIP_NSTATS * sizeof(uint64_t), h_stats);
    rc = A.stage();
    if (rc)
      return rc;
    rc = bake_probes_launch(scene, A.at<double>(positions), A.at<double>(normals), n_probes, params, HOST_SLICE, A.at<char>(ws), nullptr,
                            A.at<double>(coeff), A.at<float>(coeff_f), A.at<uint32_t>(status), A.at<uint64_t>(stats), nullptr);
    return rc ? rc : download_then_status(A, phys);
  });
}

/* ---- probe grids (rt_hip.h, rt_hip_probe_grid_* / rt_hip_probe_shade / rt_hip_probe_preview*) ------------------------------------
 * The grid's checks need no device.  The bake is the positions and rt_hip_bake_probes' launch; the preview is a ray query, the
 * first-hit albedo, the emission of what was hit, the shade and the bytes, each the call that exists. */
uint64_t grid_probes(const RtHipProbeGrid *g) { return (uint64_t)g->count[0] * g->count[1] * g->count[2]; }

/* what every grid call refuses in its grid without a device: RT_HIP_EINVAL, or RT_HIP_OK */
int check_grid(const RtHipProbeGrid *g)
{
  if (!g)
    return fail(RT_HIP_EINVAL, "grid is required");
  if (g->struct_size < sizeof(RtHipProbeGrid))
    return fail(RT_HIP_EINVAL, "grid->struct_size = %u is below the %zu of RtHipProbeGrid: start from rt_hip_probe_grid_defaults", g->struct_size,
                sizeof(RtHipProbeGrid));
  if ((g->flags & ~(uint32_t)RT_HIP_GRID_FACING) || g->reserved != 0u)
    return fail(RT_HIP_EINVAL, "unknown grid flags 0x%x or reserved not 0", g->flags);
  uint64_t n = 1;
  for (int a = 0; a < 3; a++)
  {
    if (!(g->step[a] > 0) || !std::isfinite(g->step[a]) || !std::isfinite(g->origin[a]))
      return fail(RT_HIP_EINVAL, "grid axis %d: the step %g must be finite and > 0, the origin %g finite", a, g->step[a], g->origin[a]);
    if (!std::isfinite(g->miss_color[a]))
      return fail(RT_HIP_EINVAL, "miss_color must be finite");
    if (g->count[a] == 0u)
      return fail(RT_HIP_EINVAL, "grid axis %d has no probe", a);
    n *= g->count[a]; /* (at most 2^56 before the test below: below 2^24 after two factors, or refused at the third) */
    if (n > (1u << 24))
      return fail(RT_HIP_EINVAL, "the grid has more than 2^24 probes");
  }
  return RT_HIP_OK;
}

PtGrid grid_args(const RtHipProbeGrid *g)
{
  PtGrid G;
  memset(&G, 0, sizeof G);
  for (int a = 0; a < 3; a++)
  {
    G.origin[a] = g->origin[a];
    G.step[a] = g->step[a];
    G.count[a] = g->count[a];
    G.miss_color[a] = g->miss_color[a];
  }
  G.flags = g->flags;
  return G;
}

/* a grid bake's workspace: rt_hip_bake_probes' own, then the positions */
size_t grid_bake_positions_at(uint64_t n_probes, uint64_t slice_rays) { return probe_workspace(n_probes, RT_HIP_PROBE_SPHERE, slice_rays).total; }

int check_grid_bake(const RtHipProbeGrid *grid, const RtHipProbeParams *params)
{
  if (const int rc = check_grid(grid))
    return rc;
  if (const int rc = check_probe(params, grid_probes(grid), false))
    return rc;
  if (params->mode != RT_HIP_PROBE_SPHERE)
    return fail(RT_HIP_EINVAL, "a grid is baked in RT_HIP_PROBE_SPHERE mode: its shade evaluates SH9 coefficients");
  return RT_HIP_OK;
}

/* the two calls in sequence, on the scene's device */
int bake_probe_grid_launch(const RtHipScene *scene, const RtHipProbeGrid *grid, const RtHipProbeParams *p, uint32_t slice_rays, void *d_workspace,
                           double *d_coeff, float *d_coeff_f, uint32_t *d_status, uint64_t *d_stats, hipStream_t stream)
{
  const uint64_t n = grid_probes(grid), total = n * (uint64_t)p->samples;
  double *const positions = reinterpret_cast<double *>(static_cast<char *>(d_workspace) + grid_bake_positions_at(n, std::min<uint64_t>(slice_rays, total)));
  {
    DeviceScope scope(scene->device);
    HIP_TRY(scope.status);
    if (const int rc = launched(probe_launch_grid_positions(grid_args(grid), positions, stream), "k_probe_grid_positions"))
      return rc;
  }
  return bake_probes_launch(scene, positions, nullptr, n, p, slice_rays, d_workspace, nullptr, d_coeff, d_coeff_f, d_status, d_stats, stream);
}

/* what rt_hip_probe_shade refuses without a device */
int check_shade(const RtHipProbeGrid *grid, const double *coeff, const double *points, const double *normals, uint64_t m, const void *irradiance,
                const void *color)
{
  if (const int rc = check_grid(grid))
    return rc;
  if (m > 0xFFFFFFFFull)
    return fail(RT_HIP_EINVAL, "m = %llu: a call shades fewer than 2^32 entries", (unsigned long long)m);
  if (!coeff || !points || !normals)
    return fail(RT_HIP_EINVAL, "d_coeff, d_points and d_normals are required");
  if (!irradiance && !color)
    return fail(RT_HIP_EINVAL, "one of d_irradiance and d_color is required");
  return RT_HIP_OK;
}

int shade_launch(const RtHipProbeGrid *grid, const double *d_coeff, const double *d_points, const double *d_normals, const uint32_t *d_status,
                 const float *d_albedo, const float *d_add, uint64_t m, double *d_irradiance, float *d_color, hipStream_t stream)
{
  PtProbeShade A;
  memset(&A, 0, sizeof A);
  A.grid = grid_args(grid);
  A.coeff = d_coeff;
  A.points = d_points;
  A.normals = d_normals;
  A.status = d_status;
  A.albedo = d_albedo;
  A.add = d_add;
  A.irradiance = d_irradiance;
  A.color = d_color;
  A.m = (uint32_t)m;
  return launched(probe_launch_shade(A, stream), "k_probe_shade");
}

/* a preview's workspace for n pixels in tile_px tile pixels: the centres, the query's outputs, the albedo as tiles and as an image,
 * the emission */
struct PreviewWorkspace
{
  size_t uv, status, object, point, normal, albedo_tiles, albedo, add, total;
  PreviewWorkspace(uint64_t n, uint64_t tile_px)
  {
    uv = 0;
    status = uv + stage_align(16u * n);
    object = status + stage_align(4u * n);
    point = object + stage_align(4u * n);
    normal = point + stage_align(24u * n);
    albedo_tiles = normal + stage_align(24u * n);
    albedo = albedo_tiles + stage_align(12u * tile_px);
    add = albedo + stage_align(12u * n);
    total = add + stage_align(12u * n);
  }
};

uint64_t frame_tile_pixels(int32_t width, int32_t height) { return (uint64_t)tiles_x_of(width) * tiles_y_of(height) * PT_TILE_PIXELS; }

/* what rt_hip_probe_preview refuses without a device */
int check_preview(const RtHipCamera *camera, const RtHipProbeGrid *grid, int32_t width, int32_t height, int32_t aov_samples)
{
  if (const int rc = check_grid(grid))
    return rc;
  if (!camera)
    return fail(RT_HIP_EINVAL, "camera is required");
  if (!frame_size_ok(width, height, 2))
    return fail(RT_HIP_EINVAL, "width and height must be in [2, 2^20] with fewer than 2^32 pixels");
  if (aov_samples < 1 || aov_samples > (1 << 26))
    return fail(RT_HIP_EINVAL, "aov_samples = %d must be in [1, 2^26]", aov_samples);
  return RT_HIP_OK;
}

/* The preview on `stream`, no host wait: each step is the call the header names. */
int shade_vis_launch(const RtHipProbeGrid *grid, const RtHipProbeVis *vis, const double *d_coeff, const double *d_moments, const double *d_points,
                     const double *d_normals, const uint32_t *d_status, const float *d_albedo, const float *d_add, uint64_t m, double *d_irradiance,
                     float *d_color, hipStream_t stream);

/* (vis: rt_hip_probe_preview_vis' shade, with d_moments; null: rt_hip_probe_preview's) */
int probe_preview_launch(const RtHipScene *scene, const RtHipCamera *camera, const RtHipProbeGrid *grid, const double *d_coeff, int32_t width,
                         int32_t height, int32_t aov_samples, uint64_t seed, void *d_workspace, float *d_rgb, uint8_t *d_rgb8, hipStream_t stream,
                         const RtHipProbeVis *vis = nullptr, const double *d_moments = nullptr)
{
  const uint64_t n = (uint64_t)width * (uint64_t)height;
  const PreviewWorkspace W(n, frame_tile_pixels(width, height));
  char *const ws = static_cast<char *>(d_workspace);
  double *const uv = reinterpret_cast<double *>(ws + W.uv);
  const RtHipHits hits = {reinterpret_cast<uint32_t *>(ws + W.status), nullptr, reinterpret_cast<uint32_t *>(ws + W.object), nullptr,
                          reinterpret_cast<double *>(ws + W.point), reinterpret_cast<double *>(ws + W.normal), nullptr, nullptr};
  float *const add = reinterpret_cast<float *>(ws + W.add);
  RtHipQueryParams Q;
  rt_hip_query_defaults(&Q);
  Q.source = RT_HIP_RAYS_CAMERA_UV;
  Q.camera = camera;
  /* (the camera's distance: a hint, as a render launch of that camera has it; it changes no bit) */
  Q.origin_radius = std::sqrt((camera->position[0] * camera->position[0] + camera->position[1] * camera->position[1]) +
                              camera->position[2] * camera->position[2]);
  if (const int rc = check_query(uv, true, n, &Q, &hits))
    return rc;
  {
    DeviceScope scope(scene->device);
    HIP_TRY(scope.status);
    if (const int rc = launched(probe_launch_pixel_centres((uint32_t)width, (uint32_t)height, uv, stream), "k_probe_pixel_centres"))
      return rc;
  }
  if (const int rc = query_launch(scene, uv, nullptr, n, &Q, &hits, stream))
    return rc;
  RtHipParams P;
  memset(&P, 0, sizeof P);
  P.width = width;
  P.height = height;
  P.samples = aov_samples;
  P.seed = seed;
  whole_image(P);
  const RtHipAov tiles = {reinterpret_cast<float *>(ws + W.albedo_tiles), nullptr, nullptr, nullptr, nullptr};
  const RtHipAov image = {reinterpret_cast<float *>(ws + W.albedo), nullptr, nullptr, nullptr, nullptr};
  if (const int rc = rt_hip_render_aov_tiles(scene, camera, &P, &tiles, stream))
    return rc;
  if (const int rc = rt_hip_untile_aov(&tiles, width, height, 0, 1, P.tile_count, &image, stream))
    return rc;
  DeviceScope scope(scene->device);
  HIP_TRY(scope.status);
  /* the scene's material records hold the emission, spheres then meshes: rt_hip_scene_create's numbering */
  if (const int rc = launched(probe_launch_emission(hits.object, n, scene->view.material + PT_MAT_EMISSION, PT_MAT_STRIDE, scene->view.n_spheres + scene->view.n_meshes,
                                                    add, stream), "k_probe_emission"))
    return rc;
  if (const int rc = vis ? shade_vis_launch(grid, vis, d_coeff, d_moments, hits.point, hits.normal, hits.status, image.albedo, add, n, nullptr,
                                            d_rgb, stream)
                         : shade_launch(grid, d_coeff, hits.point, hits.normal, hits.status, image.albedo, add, n, nullptr, d_rgb, stream))
    return rc;
  return d_rgb8 ? launched(probe_launch_tonemap(d_rgb, 3u * n, d_rgb8, stream), "k_probe_tonemap") : (int)RT_HIP_OK;
}

/* what the preview's host forms refuse without a device */
int check_preview_image(const RtHipCamera *camera, const RtHipProbeGrid *grid, const RtHipProbeParams *params, int32_t width, int32_t height,
                        int32_t aov_samples, const void *h_rgb, const void *h_rgb8)
{
  if (const int rc = check_grid_bake(grid, params))
    return rc;
  if (const int rc = check_preview(camera, grid, width, height, aov_samples))
    return rc;
  if (!h_rgb && !h_rgb8)
    return fail(RT_HIP_EINVAL, "one of h_rgb and h_rgb8 is required");
  return RT_HIP_OK;
}

/* The preview's host forms on a scene, its device (`phys`) current: one allocation for both workspaces, the coefficients, the frame
 * and the counters; the bake and the preview on the null stream, the copies, the device's status word. */
int preview_image_of(const RtHipScene *scene, int phys, const RtHipCamera *camera, const RtHipProbeGrid *grid, const RtHipProbeParams *params,
                     int32_t width, int32_t height, int32_t aov_samples, float *h_rgb, uint8_t *h_rgb8, double *h_coeff, uint64_t *h_stats)
{
  const uint64_t n_probes = grid_probes(grid), total = n_probes * (uint64_t)params->samples, n = (uint64_t)width * (uint64_t)height;
  const uint64_t slice = std::min<uint64_t>(HOST_SLICE, total);
  StageArena A;
  const int bake_ws = A.part(grid_bake_positions_at(n_probes, slice) + stage_align(24u * n_probes));
  const int ws = A.part(PreviewWorkspace(n, frame_tile_pixels(width, height)).total);
  const int coeff = A.part(24u * PT_PROBE_SH * n_probes, nullptr, h_coeff);
  const int rgb = A.part(12u * n, nullptr, h_rgb);
  const int rgb8 = A.part(3u * n, nullptr, h_rgb8, h_rgb8 != nullptr);
  const int stats = A.zeroed(RT_HIP_NSTATS * sizeof(uint64_t), h_stats);
  int rc = A.stage();
  if (rc)
    return rc;
  rc = bake_probe_grid_launch(scene, grid, params, HOST_SLICE, A.at<char>(bake_ws), A.at<double>(coeff), nullptr, nullptr, A.at<uint64_t>(stats),
                              nullptr);
  if (!rc)
    rc = probe_preview_launch(scene, camera, grid, A.at<double>(coeff), width, height, aov_samples, params->seed, A.at<char>(ws),
                              A.at<float>(rgb), A.at<uint8_t>(rgb8), nullptr);
  return rc ? rc : download_then_status(A, phys);
}

/* rt_hip_probe_preview_image: ... with a scene of its own on the logical device */
int probe_preview_image_impl(const RtHipSphere *spheres, size_t n_spheres, const RtHipMesh *meshes, size_t n_meshes, const RtHipCamera *camera,
                             const RtHipProbeGrid *grid, const RtHipProbeParams *params, int32_t width, int32_t height, int32_t aov_samples,
                             int device, float *h_rgb, uint8_t *h_rgb8, double *h_coeff, uint64_t *h_stats)
{
  if (const int rc = check_preview_image(camera, grid, params, width, height, aov_samples, h_rgb, h_rgb8))
    return rc;
  return with_owned_scene(spheres, n_spheres, meshes, n_meshes, device, [&](const RtHipScene *scene, int phys) {
    return preview_image_of(scene, phys, camera, grid, params, width, height, aov_samples, h_rgb, h_rgb8, h_coeff, h_stats);
  });
}

/* rt_hip_probe_preview_scene_image: ... on a scene the caller holds, on that scene's device */
int probe_preview_scene_image_impl(const RtHipScene *scene, const RtHipCamera *camera, const RtHipProbeGrid *grid, const RtHipProbeParams *params,
                                   int32_t width, int32_t height, int32_t aov_samples, float *h_rgb, uint8_t *h_rgb8, double *h_coeff,
                                   uint64_t *h_stats)
{
  if (const int rc = check_preview_image(camera, grid, params, width, height, aov_samples, h_rgb, h_rgb8))
    return rc;
  if (!scene)
    return fail(RT_HIP_EINVAL, "scene is required");
  DeviceScope scope(scene->device);
  HIP_TRY(scope.status);
  return preview_image_of(scene, scene->device, camera, grid, params, width, height, aov_samples, h_rgb, h_rgb8, h_coeff, h_stats);
}

/* ---- probe visibility (rt_hip.h, rt_hip_probe_vis_* / rt_hip_bake_probe_depth / rt_hip_probe_shade_vis / _preview_vis*) -----------
 * The depth bake is a generated-ray job whose middle is the ray query's launch instead of the radiance query's: a sibling of
 * sliced_trace with a workspace of its own, so that the lens and the radiance bake keep theirs.  The checks need no device. */
constexpr uint64_t VIS_TEXELS_MAX = 1ull << 28;

/* what every visibility call refuses in its vis without a device; n_probes: the probes whose maps the call holds */
int check_vis(const RtHipProbeVis *v, uint64_t n_probes)
{
  if (!v)
    return fail(RT_HIP_EINVAL, "vis is required");
  if (v->struct_size < sizeof(RtHipProbeVis))
    return fail(RT_HIP_EINVAL, "vis->struct_size = %u is below the %zu of RtHipProbeVis: start from rt_hip_probe_vis_defaults", v->struct_size,
                sizeof(RtHipProbeVis));
  if (v->flags != 0u || v->reserved != 0u)
    return fail(RT_HIP_EINVAL, "vis flags and reserved must be 0");
  if (v->res < PT_VIS_RES_MIN || v->res > PT_VIS_RES_MAX)
    return fail(RT_HIP_EINVAL, "vis->res = %u must be in [%u, %u]", v->res, PT_VIS_RES_MIN, PT_VIS_RES_MAX);
  if (v->sharp > PT_VIS_SHARP_MAX)
    return fail(RT_HIP_EINVAL, "vis->sharp = %u must be at most %u", v->sharp, PT_VIS_SHARP_MAX);
  if (!(v->d_max > 0) || !std::isfinite(v->d_max))
    return fail(RT_HIP_EINVAL, "vis->d_max %g must be finite and > 0", v->d_max);
  if (!(v->bias >= 0) || !std::isfinite(v->bias))
    return fail(RT_HIP_EINVAL, "vis->bias %g must be finite and >= 0", v->bias);
  if (!(v->floor > 0) || !(v->floor <= 1))
    return fail(RT_HIP_EINVAL, "vis->floor %g must be in (0, 1]", v->floor);
  if (n_probes > VIS_TEXELS_MAX || n_probes * v->res * v->res > VIS_TEXELS_MAX)
    return fail(RT_HIP_EINVAL, "%llu probes x %u x %u texels exceed 2^28", (unsigned long long)n_probes, v->res, v->res);
  return RT_HIP_OK;
}

PtProbeVis vis_args(const RtHipProbeVis *v)
{
  PtProbeVis V;
  memset(&V, 0, sizeof V);
  V.d_max = v->d_max;
  V.bias = v->bias;
  V.floor = v->floor;
  V.res = v->res;
  V.sharp = v->sharp;
  return V;
}

/* a depth bake's workspace: a slice's rays, status words and distances, then the sums, three doubles a texel and probe */
struct DepthWorkspace
{
  size_t rays, status, t, sum, total;
  DepthWorkspace(uint64_t slice, uint64_t n_probes, uint32_t res)
  {
    rays = 0;
    status = rays + stage_align(48u * slice);
    t = status + stage_align(4u * slice);
    sum = t + stage_align(8u * slice);
    total = sum + stage_align(24u * n_probes * res * res);
  }
};

/* what rt_hip_bake_probe_depth refuses without a device, but for its pointers */
int check_depth_bake(const RtHipProbeVis *vis, const RtHipProbeParams *params, uint64_t n_probes, uint32_t slice_rays, const void *d_workspace)
{
  if (const int rc = check_probe(params, n_probes, false))
    return rc;
  if (params->mode != RT_HIP_PROBE_SPHERE)
    return fail(RT_HIP_EINVAL, "depth moments are baked in RT_HIP_PROBE_SPHERE mode: a map covers every direction");
  if (const int rc = check_vis(vis, n_probes))
    return rc;
  if (slice_rays == 0u)
    return fail(RT_HIP_EINVAL, "slice_rays must be >= 1");
  return check_slice_buffers(d_workspace, nullptr);
}

/* The depth bake on `stream`, no host wait: the query's own refusal (near_R) asked for once, up front; then the sums cleared, the
 * status words marked, and per slice the probe rays, query_launch for status and t, the fold; then the resolve.  n_probes >= 1. */
int bake_probe_depth_launch(const RtHipScene *scene, const double *d_positions, uint64_t n_probes, const RtHipProbeVis *vis,
                            const RtHipProbeParams *p, uint32_t slice_rays, void *d_workspace, double *d_moments, uint32_t *d_status,
                            hipStream_t stream)
{
  const uint64_t S = (uint64_t)p->samples, total = n_probes * S, slice = std::min<uint64_t>(slice_rays, total);
  const uint64_t texels = n_probes * vis->res * vis->res;
  RtHipQueryParams Q;
  rt_hip_query_defaults(&Q);
  Q.origin_radius = p->origin_radius;
  {
    PtLaunch dry;
    if (const int rc = ray_launch_prepare(scene, Q.source, nullptr, Q.origin_radius, dry))
      return rc;
  }
  const DepthWorkspace W(slice, n_probes, vis->res);
  char *const ws = static_cast<char *>(d_workspace);
  double *const rays = reinterpret_cast<double *>(ws + W.rays), *const sum = reinterpret_cast<double *>(ws + W.sum);
  const RtHipHits hits = {reinterpret_cast<uint32_t *>(ws + W.status), reinterpret_cast<double *>(ws + W.t), nullptr, nullptr, nullptr, nullptr,
                          nullptr, nullptr};
  PtProbeRays A = probe_args(d_positions, nullptr, p);
  A.rays = rays;
  PtProbeDepthFold F;
  memset(&F, 0, sizeof F);
  F.rays = rays;
  F.t = hits.t;
  F.status = hits.status;
  F.sum = sum;
  F.probe_status = d_status;
  F.samples = A.samples;
  F.vis = vis_args(vis);
  {
    DeviceScope scope(scene->device);
    HIP_TRY(scope.status);
    HIP_TRY(hipMemsetAsync(sum, 0, 24u * texels, stream));
    if (d_status)
      HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(d_status), 1, n_probes, stream));
  }
  for (uint64_t first = 0, n; first < total; first += n)
  {
    n = std::min<uint64_t>(slice, total - first);
    {
      DeviceScope scope(scene->device);
      HIP_TRY(scope.status);
      A.k_first = first;
      A.n = (uint32_t)n;
      if (const int rc = launched(probe_launch_rays(A, stream), "k_probe_rays"))
        return rc;
    }
    if (const int rc = query_launch(scene, rays, nullptr, n, &Q, &hits, stream))
      return rc;
    DeviceScope scope(scene->device);
    HIP_TRY(scope.status);
    F.k_first = first;
    F.n = (uint32_t)n;
    F.probe_first = first / S;
    F.n_probes = (first + n - 1u) / S - F.probe_first + 1u;
    if (const int rc = launched(probe_launch_depth_fold(F, stream), "k_probe_depth_fold"))
      return rc;
  }
  if (!d_moments) /* (an update round's job, which stops at its sums) */
    return RT_HIP_OK;
  DeviceScope scope(scene->device);
  HIP_TRY(scope.status);
  return launched(probe_launch_depth_resolve(sum, texels, vis->d_max, d_moments, stream), "k_probe_depth_resolve");
}

/* a grid depth bake's workspace: the bake's own, then the positions */
size_t grid_depth_positions_at(uint64_t n_probes, uint32_t res, uint64_t slice_rays) { return DepthWorkspace(slice_rays, n_probes, res).total; }

int check_grid_depth_bake(const RtHipProbeGrid *grid, const RtHipProbeVis *vis, const RtHipProbeParams *params, uint32_t slice_rays,
                          const void *d_workspace)
{
  if (const int rc = check_grid(grid))
    return rc;
  return check_depth_bake(vis, params, grid_probes(grid), slice_rays, d_workspace);
}

/* the two calls in sequence, on the scene's device */
int bake_probe_grid_depth_launch(const RtHipScene *scene, const RtHipProbeGrid *grid, const RtHipProbeVis *vis, const RtHipProbeParams *p,
                                 uint32_t slice_rays, void *d_workspace, double *d_moments, uint32_t *d_status, hipStream_t stream)
{
  const uint64_t n = grid_probes(grid), total = n * (uint64_t)p->samples;
  double *const positions =
      reinterpret_cast<double *>(static_cast<char *>(d_workspace) + grid_depth_positions_at(n, vis->res, std::min<uint64_t>(slice_rays, total)));
  {
    DeviceScope scope(scene->device);
    HIP_TRY(scope.status);
    if (const int rc = launched(probe_launch_grid_positions(grid_args(grid), positions, stream), "k_probe_grid_positions"))
      return rc;
  }
  return bake_probe_depth_launch(scene, positions, n, vis, p, slice_rays, d_workspace, d_moments, d_status, stream);
}

int shade_vis_launch(const RtHipProbeGrid *grid, const RtHipProbeVis *vis, const double *d_coeff, const double *d_moments, const double *d_points,
                     const double *d_normals, const uint32_t *d_status, const float *d_albedo, const float *d_add, uint64_t m, double *d_irradiance,
                     float *d_color, hipStream_t stream)
{
  PtProbeShadeVis A;
  memset(&A, 0, sizeof A);
  A.shade.grid = grid_args(grid);
  A.shade.coeff = d_coeff;
  A.shade.points = d_points;
  A.shade.normals = d_normals;
  A.shade.status = d_status;
  A.shade.albedo = d_albedo;
  A.shade.add = d_add;
  A.shade.irradiance = d_irradiance;
  A.shade.color = d_color;
  A.shade.m = (uint32_t)m;
  A.vis = vis_args(vis);
  A.moments = d_moments;
  return launched(probe_launch_shade_vis(A, stream), "k_probe_shade_vis");
}

/* what the _vis preview's host forms refuse without a device */
int check_preview_vis_image(const RtHipCamera *camera, const RtHipProbeGrid *grid, const RtHipProbeVis *vis, const RtHipProbeParams *params,
                            int32_t width, int32_t height, int32_t aov_samples, const void *h_rgb, const void *h_rgb8)
{
  if (const int rc = check_preview_image(camera, grid, params, width, height, aov_samples, h_rgb, h_rgb8))
    return rc;
  return check_vis(vis, grid_probes(grid));
}

/* preview_image_of with the moments baked after the coefficients and the _vis preview */
int preview_vis_image_of(const RtHipScene *scene, int phys, const RtHipCamera *camera, const RtHipProbeGrid *grid, const RtHipProbeVis *vis,
                         const RtHipProbeParams *params, int32_t width, int32_t height, int32_t aov_samples, float *h_rgb, uint8_t *h_rgb8,
                         double *h_coeff, double *h_moments, uint64_t *h_stats)
{
  const uint64_t n_probes = grid_probes(grid), total = n_probes * (uint64_t)params->samples, n = (uint64_t)width * (uint64_t)height;
  const uint64_t slice = std::min<uint64_t>(HOST_SLICE, total);
  StageArena A;
  const int bake_ws = A.part(grid_bake_positions_at(n_probes, slice) + stage_align(24u * n_probes));
  const int depth_ws = A.part(grid_depth_positions_at(n_probes, vis->res, slice) + stage_align(24u * n_probes));
  const int ws = A.part(PreviewWorkspace(n, frame_tile_pixels(width, height)).total);
  const int coeff = A.part(24u * PT_PROBE_SH * n_probes, nullptr, h_coeff);
  const int moments = A.part(16u * n_probes * vis->res * vis->res, nullptr, h_moments);
  const int rgb = A.part(12u * n, nullptr, h_rgb);
  const int rgb8 = A.part(3u * n, nullptr, h_rgb8, h_rgb8 != nullptr);
  const int stats = A.zeroed(RT_HIP_NSTATS * sizeof(uint64_t), h_stats);
  int rc = A.stage();
  if (rc)
    return rc;
  rc = bake_probe_grid_launch(scene, grid, params, HOST_SLICE, A.at<char>(bake_ws), A.at<double>(coeff), nullptr, nullptr, A.at<uint64_t>(stats),
                              nullptr);
  if (!rc)
    rc = bake_probe_grid_depth_launch(scene, grid, vis, params, HOST_SLICE, A.at<char>(depth_ws), A.at<double>(moments), nullptr, nullptr);
  if (!rc)
    rc = probe_preview_launch(scene, camera, grid, A.at<double>(coeff), width, height, aov_samples, params->seed, A.at<char>(ws),
                              A.at<float>(rgb), A.at<uint8_t>(rgb8), nullptr, vis, A.at<double>(moments));
  return rc ? rc : download_then_status(A, phys);
}

/* ---- probe updates (rt_hip.h, rt_hip_probe_update_* / rt_hip_probe_grid_update* / rt_hip_probe_blend_*) -----------------------------
 * A round is the radiance bake's job and the depth bake's job at the positions of the round's probes, each stopped before its resolve,
 * then the blends of their sums into the grid's state and the age step.  The checks need no device. */
int check_update(const RtHipProbeUpdate *u)
{
  if (!u)
    return fail(RT_HIP_EINVAL, "upd is required");
  if (u->struct_size < sizeof(RtHipProbeUpdate))
    return fail(RT_HIP_EINVAL, "upd->struct_size = %u is below the %zu of RtHipProbeUpdate: start from rt_hip_probe_update_defaults",
                u->struct_size, sizeof(RtHipProbeUpdate));
  if (u->flags != 0u || u->reserved != 0u)
    return fail(RT_HIP_EINVAL, "update flags and reserved must be 0");
  if (u->stride == 0u || u->phase >= u->stride)
    return fail(RT_HIP_EINVAL, "stride = %u must be >= 1 and phase = %u below it", u->stride, u->phase);
  if (!(u->hysteresis >= 0) || !(u->hysteresis < 1))
    return fail(RT_HIP_EINVAL, "hysteresis %g must be in [0, 1)", u->hysteresis);
  if (!(u->fast >= 0) || !(u->fast < 1))
    return fail(RT_HIP_EINVAL, "fast %g must be in [0, 1)", u->fast);
  if (!(u->change >= 0) || !std::isfinite(u->change))
    return fail(RT_HIP_EINVAL, "change %g must be finite and >= 0", u->change);
  return RT_HIP_OK;
}

/* the round's probes of a checked update on a checked grid */
PtProbeRound round_args(const RtHipProbeGrid *grid, const RtHipProbeUpdate *u)
{
  const uint64_t n = grid_probes(grid);
  return {u->stride, u->phase, u->phase < n ? (uint32_t)((n - 1u - u->phase) / u->stride + 1u) : 0u};
}

/* a round's workspace: the bake's own for m probes, the depth bake's own (res 0: none), the m positions, the m status words */
struct UpdateWorkspace
{
  size_t bake, depth, positions, status, total;
  UpdateWorkspace(uint64_t m, uint64_t slice, uint32_t res)
  {
    bake = 0;
    depth = bake + probe_workspace(m, RT_HIP_PROBE_SPHERE, slice).total;
    positions = depth + (res ? DepthWorkspace(slice, m, res).total : 0u);
    status = positions + stage_align(24u * m);
    total = status + stage_align(4u * m);
  }
};

/* the one layout of a round's workspace, for the size the caller asks and for the launch: slices never exceed the round's m x S rays
 * (S unknown: the size is asked for slice_rays as given, which every part grows with) */
UpdateWorkspace update_workspace(uint64_t m, uint64_t slice_rays, uint64_t samples, uint32_t res)
{
  return UpdateWorkspace(m, samples ? std::min<uint64_t>(slice_rays, m * samples) : slice_rays, res);
}

/* what rt_hip_probe_grid_update refuses without a device, but for its pointers */
int check_grid_update(const RtHipProbeGrid *grid, const RtHipProbeVis *vis, const RtHipProbeParams *params, const RtHipProbeUpdate *upd,
                      uint32_t slice_rays, const void *d_workspace)
{
  if (const int rc = check_update(upd))
    return rc;
  if (const int rc = check_grid_bake(grid, params))
    return rc;
  if (vis)
    if (const int rc = check_vis(vis, grid_probes(grid)))
      return rc;
  for (int a = 0; a < 3; a++) /* (the positions grow along an axis: the last one finite, every one finite -- no ray of a round is invalid) */
    if (!std::isfinite(grid->origin[a] + (double)(grid->count[a] - 1u) * grid->step[a]))
      return fail(RT_HIP_EINVAL, "grid axis %d: the position of its last probe is not finite", a);
  if (slice_rays == 0u)
    return fail(RT_HIP_EINVAL, "slice_rays must be >= 1");
  return check_slice_buffers(d_workspace, nullptr);
}

int coeff_blend_launch(const double *d_sum, int32_t samples, const PtProbeRound &R, const RtHipProbeUpdate *upd, const uint32_t *d_age,
                       double *d_coeff, float *d_coeff_f, double *d_change, hipStream_t stream)
{
  const PtProbeCoeffBlend A = {R, d_sum, d_age, d_coeff, d_coeff_f, d_change, 1.0 / (double)samples, PT_PROBE_K_SPHERE, upd->hysteresis,
                               upd->change, upd->fast};
  return launched(probe_launch_coeff_blend(A, stream), "k_probe_coeff_blend");
}

int moment_blend_launch(const double *d_sums, const RtHipProbeVis *vis, const PtProbeRound &R, const RtHipProbeUpdate *upd,
                        const uint32_t *d_age, double *d_moments, hipStream_t stream)
{
  const PtProbeMomentBlend A = {R, d_sums, d_age, d_moments, upd->hysteresis, vis->d_max, vis->res};
  return launched(probe_launch_moment_blend(A, stream), "k_probe_moment_blend");
}

/* The round on `stream`, no host wait; R.m >= 1.  The two jobs run under a copy of the params with the round's seed and write their
 * sums into their own parts of the workspace; the radiance job marks the round's status words (the depth job sees the same rays). */
int grid_update_launch(const RtHipScene *scene, const RtHipProbeGrid *grid, const RtHipProbeVis *vis, const RtHipProbeParams *params,
                       const RtHipProbeUpdate *upd, uint32_t slice_rays, void *d_workspace, double *d_coeff, float *d_coeff_f,
                       double *d_moments, uint32_t *d_age, double *d_change, uint32_t *d_status, uint64_t *d_stats, hipStream_t stream)
{
  const PtProbeRound R = round_args(grid, upd);
  RtHipProbeParams q = *params;
  q.seed = rt_mix64(params->seed + (uint64_t)upd->round);
  const uint64_t m = R.m, slice = std::min<uint64_t>(slice_rays, m * (uint64_t)q.samples);
  const UpdateWorkspace W = update_workspace(m, slice_rays, (uint64_t)q.samples, vis ? vis->res : 0u);
  char *const ws = static_cast<char *>(d_workspace);
  double *const positions = reinterpret_cast<double *>(ws + W.positions);
  uint32_t *const round_status = reinterpret_cast<uint32_t *>(ws + W.status);
  double *const sum = reinterpret_cast<double *>(ws + W.bake + probe_workspace(m, RT_HIP_PROBE_SPHERE, slice).sum);
  {
    DeviceScope scope(scene->device);
    HIP_TRY(scope.status);
    if (const int rc = launched(probe_launch_grid_positions_strided(grid_args(grid), R, positions, stream), "k_probe_grid_positions_strided"))
      return rc;
  }
  if (const int rc = bake_probes_launch(scene, positions, nullptr, m, &q, slice_rays, ws + W.bake, nullptr, nullptr, nullptr, round_status, d_stats,
                                        stream))
    return rc;
  if (vis)
    if (const int rc = bake_probe_depth_launch(scene, positions, m, vis, &q, slice_rays, ws + W.depth, nullptr, nullptr, stream))
      return rc;
  DeviceScope scope(scene->device);
  HIP_TRY(scope.status);
  if (const int rc = coeff_blend_launch(sum, q.samples, R, upd, d_age, d_coeff, d_coeff_f, d_change, stream))
    return rc;
  if (vis)
  {
    const double *const sums = reinterpret_cast<const double *>(ws + W.depth + DepthWorkspace(slice, m, vis->res).sum);
    if (const int rc = moment_blend_launch(sums, vis, R, upd, d_age, d_moments, stream))
      return rc;
  }
  return launched(probe_launch_age_step(R, d_age, round_status, d_status, stream), "k_probe_age_step");
}

/* rt_hip_probe_grid_update_host: a scene of its own on the logical device, one allocation for the workspace, the state and the
 * counters, the round on the null stream, the copies, the device's status word */
int grid_update_host_impl(const RtHipSphere *spheres, size_t n_spheres, const RtHipMesh *meshes, size_t n_meshes, const RtHipProbeGrid *grid,
                          const RtHipProbeVis *vis, const RtHipProbeParams *params, const RtHipProbeUpdate *upd, int device, double *h_coeff,
                          float *h_coeff_f, double *h_moments, uint32_t *h_age, double *h_change, uint32_t *h_status, uint64_t *h_stats)
{
  if (const int rc = check_grid_update(grid, vis, params, upd, HOST_SLICE, nullptr))
    return rc;
  if (!h_coeff || !h_age)
    return fail(RT_HIP_EINVAL, "h_coeff and h_age are required");
  if ((vis != nullptr) != (h_moments != nullptr))
    return fail(RT_HIP_EINVAL, "vis and h_moments go together");
  const PtProbeRound R = round_args(grid, upd);
  if (R.m == 0u)
    return RT_HIP_OK; /* (no probe in the round: nothing to do, on any device or none) */
  return with_owned_scene(spheres, n_spheres, meshes, n_meshes, device, [&](const RtHipScene *scene, int phys) {
    const uint64_t n = grid_probes(grid);
    const uint32_t res = vis ? vis->res : 0u;
    StageArena A;
    const int ws = A.part(update_workspace(R.m, HOST_SLICE, (uint64_t)params->samples, res).total);
    const int coeff = A.part(24u * PT_PROBE_SH * n, h_coeff, h_coeff);
    const int coeff_f = A.part(12u * PT_PROBE_SH * n, h_coeff_f, h_coeff_f, h_coeff_f != nullptr);
    const int moments = A.part(16u * n * res * res, h_moments, h_moments, vis != nullptr);
    const int age = A.part(4u * n, h_age, h_age);
    const int change = A.part(8u * n, h_change, h_change, h_change != nullptr);
    const int status = A.part(4u * n, h_status, h_status, h_status != nullptr);
    const int stats = A.zeroed(RT_HIP_NSTATS * sizeof(uint64_t), h_stats);
    int rc = A.stage();
    if (rc)
      return rc;
    rc = grid_update_launch(scene, grid, vis, params, upd, HOST_SLICE, A.at<char>(ws), A.at<double>(coeff), A.at<float>(coeff_f),
                            A.at<double>(moments), A.at<uint32_t>(age), A.at<double>(change), A.at<uint32_t>(status), A.at<uint64_t>(stats),
                            nullptr);
    return rc ? rc : download_then_status(A, phys);
  });
}

/* rt_hip_probe_update_preview_scene_image: on a scene the caller holds, on that scene's device: one allocation for both workspaces,
 * the state, the frame and the counters; the round and the preview lit by the state it leaves on the null stream, the copies, the
 * device's status word */
int update_preview_scene_image_impl(const RtHipScene *scene, const RtHipCamera *camera, const RtHipProbeGrid *grid, const RtHipProbeVis *vis,
                                    const RtHipProbeParams *params, const RtHipProbeUpdate *upd, int32_t width, int32_t height,
                                    int32_t aov_samples, float *h_rgb, uint8_t *h_rgb8, double *h_coeff, double *h_moments, uint32_t *h_age,
                                    uint64_t *h_stats)
{
  if (const int rc = check_grid_update(grid, vis, params, upd, HOST_SLICE, nullptr))
    return rc;
  if (const int rc = check_preview(camera, grid, width, height, aov_samples))
    return rc;
  if (!h_rgb && !h_rgb8)
    return fail(RT_HIP_EINVAL, "one of h_rgb and h_rgb8 is required");
  if (!scene || !h_coeff || !h_age)
    return fail(RT_HIP_EINVAL, "scene, h_coeff and h_age are required");
  if ((vis != nullptr) != (h_moments != nullptr))
    return fail(RT_HIP_EINVAL, "vis and h_moments go together");
  DeviceScope scope(scene->device);
  HIP_TRY(scope.status);
  const PtProbeRound R = round_args(grid, upd);
  const uint64_t n_probes = grid_probes(grid), n = (uint64_t)width * (uint64_t)height;
  const uint32_t res = vis ? vis->res : 0u;
  StageArena A;
  const int update_ws = A.part(update_workspace(R.m, HOST_SLICE, (uint64_t)params->samples, res).total);
  const int ws = A.part(PreviewWorkspace(n, frame_tile_pixels(width, height)).total);
  const int coeff = A.part(24u * PT_PROBE_SH * n_probes, h_coeff, h_coeff);
  const int moments = A.part(16u * n_probes * res * res, h_moments, h_moments, vis != nullptr);
  const int age = A.part(4u * n_probes, h_age, h_age);
  const int rgb = A.part(12u * n, nullptr, h_rgb);
  const int rgb8 = A.part(3u * n, nullptr, h_rgb8, h_rgb8 != nullptr);
  const int stats = A.zeroed(RT_HIP_NSTATS * sizeof(uint64_t), h_stats);
  int rc = A.stage();
  if (rc)
    return rc;
  if (R.m != 0u)
    rc = grid_update_launch(scene, grid, vis, params, upd, HOST_SLICE, A.at<char>(update_ws), A.at<double>(coeff), nullptr, A.at<double>(moments),
                            A.at<uint32_t>(age), nullptr, nullptr, A.at<uint64_t>(stats), nullptr);
  if (!rc)
    rc = probe_preview_launch(scene, camera, grid, A.at<double>(coeff), width, height, aov_samples, params->seed, A.at<char>(ws), A.at<float>(rgb),
                              A.at<uint8_t>(rgb8), nullptr, vis, A.at<double>(moments));
  return rc ? rc : download_then_status(A, scene->device);
}

/* ---- pixel refinement (rt_hip.h, rt_hip_select_pixels / _trace_pixels / _blend_pixels) ---------------------------------------
 * select and blend are image-space calls like the upsampling: arguments checked without a device, then the device that holds the
 * first buffer.  trace_pixels is a radiance query's launch (trace_launch) whose rays the kernel forms itself: the frame's camera
 * and size in the launch, the camera's distance in origin_radius' place -- the near_R of a render launch of that camera. */
int check_select(const float *values, int32_t width, int32_t height, double lo, double hi, uint32_t flags, const void *workspace,
                 const uint32_t *indices, uint32_t capacity, const uint32_t *count)
{
  if (!frame_size_ok(width, height, 1))
    return fail(RT_HIP_EINVAL, "width and height must be in [1, 2^20] with fewer than 2^32 pixels");
  if (lo != lo || hi != hi)
    return fail(RT_HIP_EINVAL, "lo and hi must not be NaN");
  if (flags & ~(uint32_t)RT_HIP_SELECT_INVERT)
    return fail(RT_HIP_EINVAL, "unknown select flags 0x%x", flags);
  if (!values || !workspace || !count)
    return fail(RT_HIP_EINVAL, "d_values, d_workspace and d_count are required");
  if (capacity != 0u && !indices)
    return fail(RT_HIP_EINVAL, "d_indices is required with capacity > 0");
  return RT_HIP_OK;
}

int check_pixels(const RtHipCamera *camera, const void *pixels, uint64_t n, const RtHipPixelParams *p, const RtHipRadiance *out)
{
  if (!p)
    return fail(RT_HIP_EINVAL, "params is required");
  if (!out || !(out->status || out->radiance || out->samples || out->paths || out->casts))
    return fail(RT_HIP_EINVAL, "radiance: at least one output array is required");
  if (out->ray)
    return fail(RT_HIP_EINVAL, "radiance: ray must be NULL (an entry's samples have a camera ray each)");
  if (const int rc = check_integrator(p->integrator, "a pixel refinement"))
    return rc;
  if (p->samples < 1 || p->sample_first < 0 || (int64_t)p->sample_first + (int64_t)p->samples > ((int64_t)1 << 31))
    return fail(RT_HIP_EINVAL, "samples = %d, sample_first = %d: samples >= 1, sample_first >= 0, sample_first + samples <= 2^31",
                p->samples, p->sample_first);
  if (const int rc = check_max_depth(p->max_depth))
    return rc;
  if (!frame_size_ok(p->width, p->height, 2))
    return fail(RT_HIP_EINVAL, "width and height must be in [2, 2^20] with fewer than 2^32 pixels");
  if (n > 0xFFFFFFFFull)
    return fail(RT_HIP_EINVAL, "n = %llu: a call takes fewer than 2^32 entries", (unsigned long long)n);
  if (!camera)
    return fail(RT_HIP_EINVAL, "camera is required");
  if (n != 0 && !pixels)
    return fail(RT_HIP_EINVAL, "pixels is required");
  return RT_HIP_OK;
}

int pixels_launch(const RtHipScene *scene, const RtHipCamera *camera, const uint32_t *d_pixels, uint64_t n, const RtHipPixelParams *p,
                  const RtHipRadiance *d_out, uint64_t *d_stats, hipStream_t stream)
{
  PtLaunch L;
  const double *c = camera->position;
  const int rc = pooled_launch_prepare(scene, RT_HIP_RAYS_CAMERA_UV, camera, std::sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]), p->samples,
                                       p->max_depth, p->seed, d_stats, L);
  if (rc)
    return rc;
  L.width = p->width;
  L.height = p->height;
  L.w_minus_1 = (double)p->width - 1.0; /* as launch_prepare: start_sample's exact quotient */
  L.h_minus_1 = (double)p->height - 1.0;
  L.inv_w_minus_1 = 1.0 / L.w_minus_1;
  L.inv_h_minus_1 = 1.0 / L.h_minus_1;
  const PtPixels Q = {.pixels = d_pixels, .n = n, .n_pixels = (uint32_t)((uint64_t)p->width * (uint64_t)p->height),
                      .sample_first = (uint32_t)p->sample_first, .status = d_out->status, .radiance = d_out->radiance,
                      .samples = d_out->samples, .paths = reinterpret_cast<unsigned long long *>(d_out->paths),
                      .casts = reinterpret_cast<unsigned long long *>(d_out->casts)};
  const int which = pt_trace_pick(scene->view);
  return pooled_launch(scene, L, stream, pt_pixel_kernel_name_of(which), [&] { return pt_launch_pixels(L, Q, stream, which); });
}

/* rt_hip_trace_pixels_host: a scene of its own on the logical device, one allocation for the list, the counters and the requested
 * outputs, the launch on the null stream, the copies (as trace_rays_host_impl) */
int trace_pixels_host_impl(const RtHipSphere *spheres, size_t n_spheres, const RtHipMesh *meshes, size_t n_meshes, const RtHipCamera *camera,
                           const uint32_t *h_pixels, uint64_t n, const RtHipPixelParams *params, int device, const RtHipRadiance *h_out,
                           uint64_t *h_stats)
{
  int rc = check_pixels(camera, h_pixels, n, params, h_out);
  if (rc || n == 0)
    return rc;
  return with_owned_scene(spheres, n_spheres, meshes, n_meshes, device, [&](const RtHipScene *scene, int) {
    StageArena A;
    const int pixels = A.part(4u * n, h_pixels);
    RadianceStage R(A, h_out, n, params->samples, h_stats); /* (check_pixels: h_out->ray is NULL) */
    rc = A.stage();
    if (rc)
      return rc;
    const RtHipRadiance d_out = R.device(A);
    rc = pixels_launch(scene, camera, A.at<uint32_t>(pixels), n, params, &d_out, A.at<uint64_t>(R.stats), nullptr);
    return rc ? rc : R.download(A);
  });
}

/* rt_hip_*_kernel_launches of one of the four kernel lists: entry `index`'s name (null beyond the list) and launch count */
const char *kernel_launches_of(int index, uint64_t *launches, int count, const char *(*name_of)(int), unsigned long long (*launches_of)(int))
{
  if (index < 0 || index >= count)
    return nullptr;
  if (launches)
    *launches = launches_of(index);
  return name_of(index);
}

int check_blend(const uint32_t *pixels, const uint32_t *status, const double *radiance, uint64_t n, int32_t width, int32_t height,
                double new_weight, double prior_scale, const float *rgb)
{
  if (!frame_size_ok(width, height, 1))
    return fail(RT_HIP_EINVAL, "width and height must be in [1, 2^20] with fewer than 2^32 pixels");
  if (n > 0xFFFFFFFFull)
    return fail(RT_HIP_EINVAL, "n = %llu: a call takes fewer than 2^32 entries", (unsigned long long)n);
  if (!(new_weight > 0) || !std::isfinite(new_weight))
    return fail(RT_HIP_EINVAL, "new_weight %g must be finite and > 0", new_weight);
  if (!(prior_scale >= 0))
    return fail(RT_HIP_EINVAL, "prior_scale %g must be >= 0", prior_scale);
  if (!rgb)
    return fail(RT_HIP_EINVAL, "d_rgb is required");
  if (n != 0 && (!pixels || !status || !radiance))
    return fail(RT_HIP_EINVAL, "d_pixels, d_status and d_radiance are required");
  return RT_HIP_OK;
}

} // namespace

extern "C" {

const char *rt_hip_last_error(void) { return g_err; }

void rt_hip_set_cancel_flag(const volatile int *flag) { g_cancel = flag; }

int rt_hip_device_count(void) { return usable_devices(); }

int rt_hip_device_info(int device, char *name, size_t name_cap, int *compute_units)
{
  if (!have_device(device))
    return fail(RT_HIP_ENODEV, "no HIP device %d", device);
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, device));
  if (name && name_cap)
    snprintf(name, name_cap, "%s (%s)", prop.name, prop.gcnArchName);
  if (compute_units)
    *compute_units = prop.multiProcessorCount;
  return RT_HIP_OK;
}

int rt_hip_scene_create(const RtHipSphere *spheres, size_t n_spheres, const RtHipMesh *meshes,
                        size_t n_meshes, int device, RtHipScene **out_scene)
{
  return guarded("rt_hip_scene_create",
                 [&] { return scene_create_impl(spheres, n_spheres, meshes, n_meshes, device, RT_HIP_BVH_HOST, out_scene); });
}

void rt_hip_scene_options_defaults(RtHipSceneOptions *opts)
{
  if (!opts)
    return;
  opts->struct_size = (uint32_t)sizeof(RtHipSceneOptions);
  opts->bvh_builder = RT_HIP_BVH_HOST;
}

int rt_hip_scene_create_opts(const RtHipSphere *spheres, size_t n_spheres, const RtHipMesh *meshes, size_t n_meshes, int device,
                             const RtHipSceneOptions *opts, RtHipScene **out_scene)
{
  uint32_t builder = RT_HIP_BVH_HOST;
  if (opts)
  {
    if (out_scene)
      *out_scene = nullptr;
    if (opts->struct_size < sizeof(RtHipSceneOptions))
      return fail(RT_HIP_EINVAL, "scene options: struct_size %u, expected %zu (rt_hip_scene_options_defaults)", opts->struct_size,
                  sizeof(RtHipSceneOptions));
    if (opts->bvh_builder != RT_HIP_BVH_HOST && opts->bvh_builder != RT_HIP_BVH_DEVICE)
      return fail(RT_HIP_EINVAL, "scene options: bvh_builder %u is neither RT_HIP_BVH_HOST nor RT_HIP_BVH_DEVICE", opts->bvh_builder);
    builder = opts->bvh_builder;
  }
  return guarded("rt_hip_scene_create_opts",
                 [&] { return scene_create_impl(spheres, n_spheres, meshes, n_meshes, device, builder, out_scene); });
}

int rt_hip_scene_bvh_read(const RtHipScene *scene, double *h_nodes, uint32_t *h_order)
{
  if (!scene)
    return fail(RT_HIP_EINVAL, "rt_hip_scene_bvh_read: scene is NULL");
  DeviceScope on(scene->device);
  HIP_TRY(on.status);
  if (h_nodes && scene->view.n_bvh_nodes)
    HIP_TRY(hipMemcpy(h_nodes, scene->view.bvh_src, (size_t)scene->view.n_bvh_nodes * PT_BVH_SRC_DOUBLES * 8, hipMemcpyDeviceToHost));
  if (h_order && scene->view.n_triangles)
    HIP_TRY(hipMemcpy(h_order, scene->view.bvh_tri, (size_t)scene->view.n_triangles * 4, hipMemcpyDeviceToHost));
  return RT_HIP_OK;
}

int rt_hip_scene_bvh_info(const RtHipScene *scene, uint32_t *builder, uint32_t *depth, uint32_t *max_depth, uint32_t *n_nodes,
                          double *tree_cost)
{
  if (!scene)
    return fail(RT_HIP_EINVAL, "rt_hip_scene_bvh_info: scene is NULL");
  if (builder) *builder = scene->bvh_builder;
  if (depth) *depth = scene->view.bvh_depth;
  if (max_depth) *max_depth = scene->bvh_max_depth;
  if (n_nodes) *n_nodes = scene->view.n_bvh_nodes;
  if (!tree_cost)
    return RT_HIP_OK;
  *tree_cost = 0.0;
  if (scene->view.n_bvh_nodes == 0)
    return RT_HIP_OK;
  return guarded("rt_hip_scene_bvh_info", [&]() -> int {
    std::vector<double> nodes((size_t)scene->view.n_bvh_nodes * PT_BVH_SRC_DOUBLES);
    const int rc = rt_hip_scene_bvh_read(scene, nodes.data(), nullptr);
    if (rc)
      return rc;
    *tree_cost = BvhSweep::tree_cost_of(nodes);
    return RT_HIP_OK;
  });
}

double rt_hip_scene_bvh_build_seconds(const RtHipScene *scene) { return scene ? scene->bvh_build_seconds : 0.0; }

int rt_hip_set_bvh_builder(int builder) { return set_bvh_builder_impl(builder); }

void rt_hip_release_cache(void) { release_cache_impl(); }

void rt_hip_last_image_phases(double seconds[3])
{
  if (seconds)
    last_phases_impl(seconds);
}

int rt_hip_set_device_map(const int *map, int n)
{
  return guarded("rt_hip_set_device_map", [&] { return set_device_map_impl(map, n); });
}

uint64_t rt_hip_cache_builds(void) { return cache_builds_impl(); }

uint64_t rt_hip_cache_updates(void) { return cache_updates_impl(); }

void rt_hip_set_scene_updates(int on) { set_scene_updates_impl(on); }

void rt_hip_set_material_updates(int on) { set_material_updates_impl(on); }

int rt_hip_set_bvh_rebuild_ratio(double max_ratio) { return set_bvh_rebuild_ratio_impl(max_ratio); }

uint64_t rt_hip_cache_rebuilds(void) { return cache_rebuilds_impl(); }

int rt_hip_render_image(const RtHipSphere *spheres, size_t n_spheres, const RtHipMesh *meshes,
                        size_t n_meshes, const RtHipCamera *camera, const RtHipParams *params,
                        int n_devices, float *h_image_rgb, uint8_t *h_image_rgb8, uint64_t *h_stats,
                        double *kernel_seconds)
{
  return guarded("rt_hip_render_image", [&] {
    return render_image_impl(spheres, n_spheres, meshes, n_meshes, camera, params, n_devices, h_image_rgb, h_image_rgb8, h_stats,
                             kernel_seconds);
  });
}

void rt_hip_scene_destroy(RtHipScene *scene)
{
  if (!scene)
    return;
  {
    DeviceScope scope(scene->device);
    for (TableSet &t : scene->tables)
    {
      (void)table_set_wait(t);
      table_set_free(t);
    }
    if (scene->park_ws)
    { /* every launch of this scene must be past its last ring access before the pool can go */
      (void)hipDeviceSynchronize();
      park_drop_ws(scene->device);
    }
    if (scene->refit_by_level)
      (void)hipFree(scene->refit_by_level);
    if (scene->bvh_side)
      (void)hipFree(scene->bvh_side);
    if (scene->cost_ws)
      (void)hipFree(scene->cost_ws);
    (void)hipFree(scene->blob);
  }
  delete scene;
}

int rt_hip_scene_device(const RtHipScene *scene) { return scene ? scene->device : -1; }

size_t rt_hip_scene_primitives(const RtHipScene *scene)
{
  return scene ? (size_t)scene->view.n_spheres + scene->view.n_triangles : 0;
}

int rt_hip_scene_hull_facets(const RtHipScene *scene, uint32_t *n_plus, uint32_t *n_minus)
{
  if (!scene || !n_plus || !n_minus)
    return fail(RT_HIP_EINVAL, "rt_hip_scene_hull_facets: null argument");
  *n_plus = *n_minus = 0;
  const size_t n = scene->view.n_triangles;
  if (n == 0 || !scene->hull_flags)
    return 0;
  return guarded("rt_hip_scene_hull_facets", [&]() -> int {
    std::vector<uint32_t> obj(n);
    DeviceScope on(scene->device);
    HIP_TRY(on.status);
    HIP_TRY(hipMemcpy(obj.data(), scene->view.tri_object, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; i++)
    {
      *n_plus += (obj[i] & PT_HULL_PLUS) ? 1u : 0u;
      *n_minus += (obj[i] & PT_HULL_MINUS) ? 1u : 0u;
    }
    return 0;
  });
}

/* ---- moving the triangles in place: new records and a refitted hierarchy (scene_update.hip), then the scalars and flags that
 * scene_create_impl derives from them, by bvh_build.h's one text (scene_mesh_bounds).  Nothing of the scene is written before every refusal has been
 * ruled out; once writing has begun a HIP failure leaves the scene unusable. */
namespace
{

/* [p, p + bytes) meets memory the scene owns: the blob, or the side allocation a rebuild made for a larger tree */
bool lies_inside_scene(const RtHipScene *scene, const void *ptr, size_t bytes)
{
  const char *p = static_cast<const char *>(ptr);
  auto meets = [&](const void *base, size_t size) {
    const char *b = static_cast<const char *>(base);
    return b && p + bytes > b && p < b + size;
  };
  return meets(scene->blob, scene->blob_bytes) || meets(scene->bvh_side, scene->bvh_side_bytes);
}

/* The device cost of the tree as it was last built: a rebuild sets it; for a created scene it is taken here, at the first
 * request -- and an update asks before its first refit, so it is never a refitted tree's.  Caller holds table_mutex and has the
 * scene's device current. */
/* The cost of `nodes` (the scene's own, or a tree still in its builder's workspace) through the workspace the scene keeps.  Every
 * cost call waits for its result, so a workspace that is too small is free to be replaced.  Caller holds table_mutex and has the
 * scene's device current. */
int scene_cost_of(const RtHipScene *scene, const double *nodes, uint32_t n_nodes, double *cost)
{
  if (n_nodes > scene->cost_ws_nodes)
  {
    DeviceBuffer ws;
    const size_t bytes = scene_tree_cost_ws_doubles(n_nodes) * sizeof(double);
    if (ws.alloc(bytes) != hipSuccess)
      return fail(RT_HIP_ENOMEM, "the cost kernel's workspace (%zu bytes)", bytes);
    if (scene->cost_ws)
      (void)hipFree(scene->cost_ws);
    scene->cost_ws = ws.at<double>();
    scene->cost_ws_nodes = n_nodes;
    ws.ptr = nullptr; /* the scene's now */
  }
  HIP_TRY(scene_tree_cost(nodes, n_nodes, scene->cost_ws, cost));
  return RT_HIP_OK;
}

int scene_built_cost(const RtHipScene *scene, double *cost)
{
  if (!scene->built_cost_known)
  {
    double c = 0.0;
    if (const int rc = scene_cost_of(scene, scene->view.bvh_src, scene->view.n_bvh_nodes, &c))
      return rc;
    scene->built_cost = c;
    scene->built_cost_known = true;
  }
  if (cost)
    *cost = scene->built_cost;
  return RT_HIP_OK;
}

/* A caller's device array that an update reads (`bytes` of it): device memory of the scene's device, outside what the scene owns */
int check_update_input(const RtHipScene *scene, const void *ptr, size_t bytes, const char *name)
{
  int device = -1;
  if (device_of(ptr, name, &device) != RT_HIP_OK || device != scene->device)
    return fail(RT_HIP_EINVAL, "%s is not device memory of the scene's device %d", name, scene->device);
  if (lies_inside_scene(scene, ptr, bytes))
    return fail(RT_HIP_EINVAL, "%s lies inside the scene", name);
  return RT_HIP_OK;
}

/* The updates' one workspace: 256 bytes for the reductions' words, then (host form) the caller's array staged behind them.
 * *d_in is the array on the device either way. */
int stage_update_input(const double *in, size_t bytes, bool on_host, DeviceBuffer &ws, unsigned long long **words, const double **d_in)
{
  const size_t words_bytes = 256, total = words_bytes + (on_host ? bytes : 0);
  static_assert(SCENE_UPDATE_WORDS * 8 <= 256 && SCENE_SPHERE_WORDS * 8 <= 256 && SCENE_MATERIAL_WORDS * 8 <= 256, "the reductions' words");
  if (ws.alloc(total) != hipSuccess)
    return fail(RT_HIP_ENOMEM, "update workspace (%zu KB)", total >> 10);
  *words = ws.at<unsigned long long>();
  *d_in = on_host ? ws.at<double>(words_bytes) : in;
  if (on_host)
    HIP_TRY(hipMemcpy(ws.at<char>(words_bytes), in, bytes, hipMemcpyHostToDevice));
  return RT_HIP_OK;
}

int scene_update_impl(RtHipScene *scene, const double *positions, size_t n_triangles, bool on_host)
{
  if (!positions)
    return fail(RT_HIP_EINVAL, "positions are required");
  if (const int rc = scene_usable(scene, "rt_hip_scene_update_vertices"))
    return rc;
  const size_t n = scene->view.n_triangles;
  if (n == 0)
    return fail(RT_HIP_EINVAL, "the scene has no triangles to move");
  if (n_triangles != n)
    return fail(RT_HIP_EINVAL, "%zu triangles given, the scene has %zu: an update keeps the count", n_triangles, n);
  SceneWrite w(scene, "its vertices move");
  HIP_TRY(w.scope.status);
  if (!on_host)
    if (const int rc = check_update_input(scene, positions, 72 * n, "d_positions"))
      return rc;
  w.lock.lock();
  if (const int rc = w.idle())
    return rc;
  const auto t0 = std::chrono::steady_clock::now();
  DeviceBuffer ws;
  unsigned long long *words = nullptr;
  const double *d_pos = nullptr;
  if (const int rc = stage_update_input(positions, 72 * n, on_host, ws, &words, &d_pos))
    return rc;
  SceneUpdateCheck chk;
  HIP_TRY(scene_update_check(d_pos, (uint32_t)n, words, &chk));
  if (!(chk.max_len <= 1e300)) /* scene_create_impl's rule */
    return fail(RT_HIP_EINVAL, "a new position has a non-finite coordinate");

  /* ---- the cost of the tree as built, while it still is that tree; the topology's levels, at the first update ---- */
  if (const int rc = scene_built_cost(scene, nullptr))
    return rc;
  const uint32_t n_nodes = scene->view.n_bvh_nodes;
  if (!scene->refit_by_level)
  {
    std::vector<double> nodes((size_t)n_nodes * PT_BVH_SRC_DOUBLES);
    std::vector<uint32_t> by_level, level_begin;
    HIP_TRY(hipMemcpy(nodes.data(), scene->view.bvh_src, nodes.size() * 8, hipMemcpyDeviceToHost));
    if (n_nodes == 0 || !BvhRefit::levels(nodes.data(), n_nodes, by_level, level_begin))
      return fail(RT_HIP_ERUNTIME, "the hierarchy numbers a child below its parent: it cannot be refitted");
    DeviceBuffer d_levels;
    if (d_levels.alloc(by_level.size() * 4) != hipSuccess)
      return fail(RT_HIP_ENOMEM, "the hierarchy's level array (%zu KB)", (by_level.size() * 4) >> 10);
    HIP_TRY(hipMemcpy(d_levels.ptr, by_level.data(), by_level.size() * 4, hipMemcpyHostToDevice));
    scene->refit_by_level = d_levels.at<uint32_t>();
    d_levels.ptr = nullptr; /* the scene's now */
    scene->refit_level_begin.swap(level_begin);
  }

  if (const int rc = w.drain())
    return rc;

  /* ---- writing begins ---- */
  w.stale();
  SceneUpdateArrays arr;
  arr.n_tri = (uint32_t)n;
  arr.n_nodes = n_nodes;
  arr.tri_geom = const_cast<double *>(scene->view.tri_geom);
  arr.tri_normal = const_cast<double *>(scene->view.tri_normal);
  arr.entry_tri = const_cast<double *>(scene->view.entry_src) + PT_ENTRY_SRC_STRIDE * (size_t)scene->view.n_spheres;
  arr.tri_object = const_cast<uint32_t *>(scene->view.tri_object);
  arr.bvh_src = const_cast<double *>(scene->view.bvh_src);
  arr.bvh_tri = scene->view.bvh_tri;
  arr.tri_geom_leaf = const_cast<double *>(scene->view.tri_geom_leaf);
  double mesh_c[3], r2 = 0;
  scene_mesh_centre(chk.lo, chk.hi, mesh_c);
  hipError_t e = scene_update_triangles(arr, d_pos, mesh_c, words, &r2);
  if (e != hipSuccess)
    return w.broke(e, "updating the triangle records");
  e = scene_update_refit(arr, scene->refit_by_level, scene->refit_level_begin.data(), scene->refit_level_begin.size() - 1);
  if (e != hipSuccess)
    return w.broke(e, "refitting the hierarchy");

  /* ---- the derived scalars and the hull flags (k_update_triangles cleared the bits), by creation's text ---- */
  SceneMeshBounds mb;
  scene_mesh_bounds(chk.lo, chk.hi, r2, &mb);
  take_mesh_bounds(scene, mb);
  scene->reach_triangles = chk.max_len; /* kept: a later update of the spheres joins it with their part again */
  scene->reach = std::fmax(scene->reach_spheres, scene->reach_triangles);
  e = scene_hull_flags(scene, mb.tau);
  if (e != hipSuccess)
    return w.broke(e, "hull flags");
  e = hipStreamSynchronize(nullptr);
  if (e != hipSuccess)
    return w.broke(e, "waiting for the update");
  scene->updates++;
  scene->last_update_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  return RT_HIP_OK;
}

/* ---- moving the spheres in place: the sphere records of entry_src and geom4 rewritten by k_update_spheres (scene_update.hip), then
 * the scalars scene_create_impl derives from the spheres, by bvh_build.h's one text.  The same discipline as above: the
 * kernel's first run writes nothing of the scene (the maxima, and whether every radius is acceptable); only when no refusal is
 * left does its second run write.  The table sets go stale as after a vertex update: the filter is made of these records. */
int scene_update_spheres_impl(RtHipScene *scene, const double *spheres, size_t n_spheres, bool on_host)
{
  if (!spheres)
    return fail(RT_HIP_EINVAL, "spheres are required");
  if (const int rc = scene_usable(scene, "rt_hip_scene_update_spheres"))
    return rc;
  const size_t n = scene->view.n_spheres;
  if (n == 0)
    return fail(RT_HIP_EINVAL, "the scene has no spheres to move");
  if (n_spheres != n)
    return fail(RT_HIP_EINVAL, "%zu spheres given, the scene has %zu: an update keeps the count", n_spheres, n);
  const size_t in_bytes = SCENE_SPHERE_IN * 8 * n;
  SceneWrite w(scene, "its spheres move");
  HIP_TRY(w.scope.status);
  if (!on_host)
    if (const int rc = check_update_input(scene, spheres, in_bytes, "d_spheres"))
      return rc;
  w.lock.lock();
  if (const int rc = w.idle())
    return rc;
  const auto t0 = std::chrono::steady_clock::now();
  DeviceBuffer ws;
  unsigned long long *words = nullptr;
  const double *d_in = nullptr;
  if (const int rc = stage_update_input(spheres, in_bytes, on_host, ws, &words, &d_in))
    return rc;
  SceneSphereBounds sb;
  bool radii_ok = false;
  HIP_TRY(scene_update_spheres_check(d_in, (uint32_t)n, words, &sb, &radii_ok));
  if (!radii_ok) /* scene_create_impl's rule */
    return fail(RT_HIP_ELIMIT, "a sphere's |radius| is outside [1e-100, 1e100]");
  /* the leading walls: the first records read back, and bvh_build.h's text on the host */
  {
    double lead[SCENE_SPHERE_IN * SCENE_SPHERE_WALLS];
    const size_t n_lead = n < SCENE_SPHERE_WALLS ? n : (size_t)SCENE_SPHERE_WALLS;
    if (on_host)
      memcpy(lead, spheres, SCENE_SPHERE_IN * 8 * n_lead);
    else
      HIP_TRY(hipMemcpy(lead, d_in, SCENE_SPHERE_IN * 8 * n_lead, hipMemcpyDeviceToHost));
    scene_sphere_leading_walls(lead, n_lead, &sb);
  }

  if (const int rc = w.drain())
    return rc;

  /* ---- writing begins ---- */
  w.stale();
  hipError_t e = scene_update_spheres_write(d_in, (uint32_t)n, const_cast<double *>(scene->view.entry_src),
                                            const_cast<double *>(scene->view.geom4));
  if (e != hipSuccess)
    return w.broke(e, "updating the sphere records");
  e = hipStreamSynchronize(nullptr);
  if (e != hipSuccess)
    return w.broke(e, "waiting for the update");
  take_sphere_bounds(scene, sb);
  scene->reach = std::fmax(scene->reach_spheres, scene->reach_triangles);
  scene->updates++;
  scene->last_update_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  return RT_HIP_OK;
}

/* ---- changing the materials in place: the `material` records and color_raw rewritten by k_update_materials (scene_update.hip),
 * then the scalars scene_create_impl derives from the materials, by bvh_build.h's one text.  The same discipline as above: the
 * kernel's first run writes nothing of the scene (the scalars, and whether every material is acceptable); only when no refusal is
 * left does its second run write.  The table sets STAY VALID (no stale()): pt_launch_build_tables reads entry_src, bvh_src and
 * tri_geom / tri_geom_leaf alone -- filter records, fp32 nodes and tri32 records hold nothing a material decides.  The host form
 * stages the materials and, where given, the flags behind them in the one workspace. */
int scene_update_materials_impl(RtHipScene *scene, const double *materials, const uint32_t *flags, size_t n_objects, bool on_host)
{
  if (const int rc = scene_usable(scene, "rt_hip_scene_update_materials"))
    return rc;
  if (!materials)
    return fail(RT_HIP_EINVAL, "materials are required");
  const size_t n = (size_t)scene->view.n_spheres + scene->view.n_meshes;
  if (n == 0)
    return fail(RT_HIP_EINVAL, "the scene has no objects whose materials could change");
  if (n_objects != n)
    return fail(RT_HIP_EINVAL, "%zu objects given, the scene has %zu: an update keeps the count", n_objects, n);
  const size_t mat_bytes = SCENE_MATERIAL_IN * 8 * n, flag_bytes = flags ? 4 * n : 0;
  SceneWrite w(scene, "its materials change");
  HIP_TRY(w.scope.status);
  if (!on_host)
  {
    if (const int rc = check_update_input(scene, materials, mat_bytes, "d_materials"))
      return rc;
    if (flags)
      if (const int rc = check_update_input(scene, flags, flag_bytes, "d_flags"))
        return rc;
  }
  w.lock.lock();
  if (const int rc = w.idle())
    return rc;
  const auto t0 = std::chrono::steady_clock::now();
  DeviceBuffer ws;
  unsigned long long *words = nullptr;
  const double *d_in = nullptr;
  const uint32_t *d_flags = flags;
  if (on_host && flags)
  { /* one staged array: the doubles, then the words */
    std::vector<double> both(SCENE_MATERIAL_IN * n + (n + 1) / 2);
    memcpy(both.data(), materials, mat_bytes);
    memcpy(both.data() + SCENE_MATERIAL_IN * n, flags, flag_bytes);
    if (const int rc = stage_update_input(both.data(), both.size() * 8, true, ws, &words, &d_in))
      return rc;
    d_flags = reinterpret_cast<const uint32_t *>(d_in + SCENE_MATERIAL_IN * n);
  }
  else if (const int rc = stage_update_input(materials, mat_bytes, on_host, ws, &words, &d_in))
    return rc;
  SceneMaterialBounds mb;
  bool materials_ok = false;
  HIP_TRY(scene_update_materials_check(d_in, d_flags, (uint32_t)n, scene->view.material, words, &mb, &materials_ok));
  if (!materials_ok) /* scene_create_impl's rule */
    return fail(RT_HIP_EINVAL, "a material is refused: colour must be finite and >= 0, emission finite (both at most 1e100)");

  if (const int rc = w.drain())
    return rc;

  /* ---- writing begins ---- */
  hipError_t e = scene_update_materials_write(d_in, d_flags, (uint32_t)n, const_cast<double *>(scene->view.material),
                                              const_cast<double *>(scene->view.color_raw));
  if (e != hipSuccess)
    return w.broke(e, "updating the material records");
  e = hipStreamSynchronize(nullptr);
  if (e != hipSuccess)
    return w.broke(e, "waiting for the update");
  take_material_bounds(scene, mb);
  scene->updates++;
  scene->last_update_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  return RT_HIP_OK;
}

/* ---- the tree priced on the device, and the topology rebuilt in place (rt_hip.h states both contracts) ---- */
int scene_cost_impl(const RtHipScene *scene, double *cost)
{
  if (!scene || !cost)
    return fail(RT_HIP_EINVAL, "rt_hip_scene_bvh_cost: scene and cost are required");
  *cost = 0.0;
  if (const int rc = scene_usable(scene, "rt_hip_scene_bvh_cost"))
    return rc;
  DeviceScope scope(scene->device);
  HIP_TRY(scope.status);
  std::lock_guard<std::mutex> lock(scene->table_mutex);
  return scene_cost_of(scene, scene->view.bvh_src, scene->view.n_bvh_nodes, cost);
}

int cost_nodes_host_impl(const double *h_nodes, size_t n_nodes, int device, double *cost)
{
  if (!cost || (!h_nodes && n_nodes > 0) || n_nodes >= ((size_t)1 << (31 - PT_BVH_COUNT_BITS)))
    return fail(RT_HIP_EINVAL, "rt_hip_bvh_cost_nodes_host: cost is required, nodes where n_nodes > 0, and n_nodes < 2^%d",
                31 - PT_BVH_COUNT_BITS);
  *cost = 0.0;
  if (n_nodes == 0)
    return RT_HIP_OK;
  return on_logical_device(device, [&](int) -> int {
    DeviceBuffer staged;
    const size_t bytes = n_nodes * PT_BVH_SRC_DOUBLES * 8;
    if (staged.alloc(bytes) != hipSuccess)
      return fail(RT_HIP_ENOMEM, "the staged nodes (%zu KB)", bytes >> 10);
    HIP_TRY(hipMemcpy(staged.ptr, h_nodes, bytes, hipMemcpyHostToDevice));
    HIP_TRY(scene_tree_cost(staged.at<double>(), (uint32_t)n_nodes, nullptr, cost));
    return RT_HIP_OK;
  });
}

/* `w` holds table_mutex and has the scene's device current; a NULL, unusable or triangle-less scene is ruled out */
int scene_rebuild_locked(SceneWrite &w)
{
  RtHipScene *scene = w.scene;
  if (const int rc = w.idle())
    return rc;
  const auto t0 = std::chrono::steady_clock::now();

  /* ---- the build, in its own workspace; the new tree priced where it lies ---- */
  BvhDeviceTree dtree;
  if (const int rc = build_device_tree(scene->view.tri_geom, scene->view.n_triangles, &dtree))
    return rc;
  double cost = 0.0;
  if (const int rc = scene_cost_of(scene, dtree.nodes, dtree.n_nodes, &cost))
    return rc;

  /* ---- room for it: in place while the count fits the capacity, else a side allocation ---- */
  const size_t src_bytes = (size_t)dtree.n_nodes * PT_BVH_SRC_DOUBLES * 8, f32_bytes = (size_t)dtree.n_nodes * PT_BVH_NODE_WORDS * 4;
  DeviceBuffer side;
  const size_t side_bytes = pad256(src_bytes) + pad256(f32_bytes);
  if (dtree.n_nodes > scene->bvh_node_capacity && side.alloc(side_bytes) != hipSuccess)
    return fail(RT_HIP_ENOMEM, "the side allocation of a larger hierarchy (%zu KB)", side_bytes >> 10);
  if (const int rc = w.drain())
    return rc;

  /* ---- installing begins ---- */
  if (scene->refit_by_level) /* the old topology's levels: the next vertex update makes the new one's */
    (void)hipFree(scene->refit_by_level);
  scene->refit_by_level = nullptr;
  scene->refit_level_begin.clear();
  while (scene->tables.size() > 1) /* the owned sets hold fp32 nodes of the old count: the next launch that needs one allocates it anew */
  {
    table_set_free(scene->tables.back());
    scene->tables.pop_back();
  }
  if (side)
  {
    if (scene->bvh_side)
      (void)hipFree(scene->bvh_side);
    scene->bvh_side = side.ptr;
    scene->bvh_side_bytes = side_bytes;
    side.ptr = nullptr; /* the scene's now */
    scene->view.bvh_src = reinterpret_cast<const double *>(scene->bvh_side);
    scene->view.bvh_nodes = reinterpret_cast<float *>(static_cast<char *>(scene->bvh_side) + pad256(src_bytes));
    scene->bvh_node_capacity = dtree.n_nodes;
  }
  for (TableSet &t : scene->tables)
    t.bvh_nodes = scene->view.bvh_nodes; /* (set 0 alone is left: its nodes are the view's) */
  w.stale();
  const hipError_t e = install_device_tree(scene, dtree);
  if (e != hipSuccess)
    return w.broke(e, "installing the rebuilt hierarchy");
  scene->built_cost = cost;
  scene->built_cost_known = true;
  scene->rebuilds++;
  scene->last_rebuild_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  return RT_HIP_OK;
}

int scene_rebuild_impl(RtHipScene *scene)
{
  if (const int rc = scene_usable(scene, "rt_hip_scene_rebuild_bvh"))
    return rc;
  if (scene->view.n_triangles == 0)
    return fail(RT_HIP_EINVAL, "the scene has no triangles: there is no hierarchy to rebuild");
  SceneWrite w(scene, "its hierarchy is rebuilt");
  HIP_TRY(w.scope.status);
  w.lock.lock();
  return scene_rebuild_locked(w);
}

/* max_ratio as rt_hip_scene_maintain_bvh takes it: finite and >= 1 */
bool rebuild_ratio_ok(double r) { return r >= 1.0 && r < HUGE_VAL; }

int scene_maintain_impl(RtHipScene *scene, double max_ratio, double *cost_ratio, int *rebuilt)
{
  if (cost_ratio) *cost_ratio = 0.0;
  if (rebuilt) *rebuilt = 0;
  if (!rebuild_ratio_ok(max_ratio))
    return fail(RT_HIP_EINVAL, "rt_hip_scene_maintain_bvh: max_ratio must be finite and >= 1");
  if (const int rc = scene_usable(scene, "rt_hip_scene_maintain_bvh"))
    return rc;
  if (scene->view.n_triangles == 0)
    return fail(RT_HIP_EINVAL, "the scene has no triangles: there is no hierarchy to maintain");
  SceneWrite w(scene, "its hierarchy is rebuilt");
  HIP_TRY(w.scope.status);
  w.lock.lock(); /* held across pricing and rebuild */
  double built = 0.0, cost = 0.0;
  if (const int rc = scene_built_cost(scene, &built))
    return rc;
  if (const int rc = scene_cost_of(scene, scene->view.bvh_src, scene->view.n_bvh_nodes, &cost))
    return rc;
  const double ratio = built == 0.0 ? 1.0 : cost / built;
  if (cost_ratio) *cost_ratio = ratio;
  if (!(ratio > max_ratio))
    return RT_HIP_OK;
  const int rc = scene_rebuild_locked(w);
  if (rc == RT_HIP_OK && rebuilt)
    *rebuilt = 1;
  return rc;
}

} // namespace

int rt_hip_scene_bvh_cost(const RtHipScene *scene, double *cost)
{
  return guarded("rt_hip_scene_bvh_cost", [&] { return scene_cost_impl(scene, cost); });
}

int rt_hip_bvh_cost_nodes_host(const double *h_nodes, size_t n_nodes, int device, double *cost)
{
  return guarded("rt_hip_bvh_cost_nodes_host", [&] { return cost_nodes_host_impl(h_nodes, n_nodes, device, cost); });
}

int rt_hip_scene_rebuild_bvh(RtHipScene *scene)
{
  return guarded("rt_hip_scene_rebuild_bvh", [&] { return scene_rebuild_impl(scene); });
}

int rt_hip_scene_rebuild_info(const RtHipScene *scene, uint64_t *rebuilds, double *last_seconds, double *built_cost)
{
  if (!scene)
    return fail(RT_HIP_EINVAL, "rt_hip_scene_rebuild_info: scene is NULL");
  if (rebuilds) *rebuilds = scene->rebuilds;
  if (last_seconds) *last_seconds = scene->last_rebuild_seconds;
  if (!built_cost)
    return RT_HIP_OK;
  *built_cost = 0.0;
  if (scene->view.n_bvh_nodes == 0)
    return RT_HIP_OK;
  if (const int rc = scene_usable(scene, "rt_hip_scene_rebuild_info"))
    return rc;
  return guarded("rt_hip_scene_rebuild_info", [&]() -> int {
    DeviceScope scope(scene->device);
    HIP_TRY(scope.status);
    std::lock_guard<std::mutex> lock(scene->table_mutex);
    return scene_built_cost(scene, built_cost);
  });
}

int rt_hip_scene_maintain_bvh(RtHipScene *scene, double max_ratio, double *cost_ratio, int *rebuilt)
{
  return guarded("rt_hip_scene_maintain_bvh", [&] { return scene_maintain_impl(scene, max_ratio, cost_ratio, rebuilt); });
}

int rt_hip_scene_update_spheres(RtHipScene *scene, const double *d_spheres, size_t n_spheres)
{
  return guarded("rt_hip_scene_update_spheres", [&] { return scene_update_spheres_impl(scene, d_spheres, n_spheres, false); });
}

int rt_hip_scene_update_spheres_host(RtHipScene *scene, const double *h_spheres, size_t n_spheres)
{
  return guarded("rt_hip_scene_update_spheres_host", [&] { return scene_update_spheres_impl(scene, h_spheres, n_spheres, true); });
}

int rt_hip_scene_update_materials(RtHipScene *scene, const double *d_materials, const uint32_t *d_flags, size_t n_objects)
{
  return guarded("rt_hip_scene_update_materials", [&] { return scene_update_materials_impl(scene, d_materials, d_flags, n_objects, false); });
}

int rt_hip_scene_update_materials_host(RtHipScene *scene, const double *h_materials, const uint32_t *h_flags, size_t n_objects)
{
  return guarded("rt_hip_scene_update_materials_host", [&] { return scene_update_materials_impl(scene, h_materials, h_flags, n_objects, true); });
}

int rt_hip_scene_read_materials(const RtHipScene *scene, double *material, double *color_raw)
{
  if (!scene)
    return fail(RT_HIP_EINVAL, "rt_hip_scene_read_materials: scene is NULL");
  const size_t n = (size_t)scene->view.n_spheres + scene->view.n_meshes;
  if (n == 0)
    return RT_HIP_OK;
  DeviceScope on(scene->device);
  HIP_TRY(on.status);
  if (material) HIP_TRY(hipMemcpy(material, scene->view.material, PT_MAT_STRIDE * 8 * n, hipMemcpyDeviceToHost));
  if (color_raw) HIP_TRY(hipMemcpy(color_raw, scene->view.color_raw, 3 * 8 * n, hipMemcpyDeviceToHost));
  return RT_HIP_OK;
}

int rt_hip_scene_material_bounds(const RtHipScene *scene, double *max_emission, uint32_t *any_refract, uint32_t *any_checker,
                                 uint32_t *any_mirror_glass)
{
  if (!scene)
    return fail(RT_HIP_EINVAL, "rt_hip_scene_material_bounds: scene is NULL");
  if (max_emission) *max_emission = scene->max_emission;
  if (any_refract) *any_refract = scene->view.any_refract;
  if (any_checker) *any_checker = scene->view.any_checker;
  if (any_mirror_glass) *any_mirror_glass = scene->view.any_mirror_glass;
  return RT_HIP_OK;
}

int rt_hip_scene_memory(const RtHipScene *scene, const void **base, size_t *bytes)
{
  if (!scene)
    return fail(RT_HIP_EINVAL, "rt_hip_scene_memory: scene is NULL");
  if (base) *base = scene->blob;
  if (bytes) *bytes = scene->blob_bytes;
  return RT_HIP_OK;
}

int rt_hip_scene_read_spheres(const RtHipScene *scene, double *entry, double *geom4)
{
  if (!scene)
    return fail(RT_HIP_EINVAL, "rt_hip_scene_read_spheres: scene is NULL");
  const size_t n = scene->view.n_spheres;
  if (n == 0)
    return RT_HIP_OK;
  DeviceScope on(scene->device);
  HIP_TRY(on.status);
  if (entry) HIP_TRY(hipMemcpy(entry, scene->view.entry_src, PT_ENTRY_SRC_STRIDE * 8 * n, hipMemcpyDeviceToHost));
  if (geom4) HIP_TRY(hipMemcpy(geom4, scene->view.geom4, PT_GEOM_STRIDE * 8 * n, hipMemcpyDeviceToHost));
  return RT_HIP_OK;
}

int rt_hip_scene_sphere_bounds(const RtHipScene *scene, double *reach_spheres, double *max_center, uint32_t *wide_range, uint32_t *n_big,
                               double big_r[8], double big_c[8])
{
  if (!scene)
    return fail(RT_HIP_EINVAL, "rt_hip_scene_sphere_bounds: scene is NULL");
  if (reach_spheres) *reach_spheres = scene->reach_spheres;
  if (max_center) *max_center = scene->max_center;
  if (wide_range) *wide_range = scene->view.wide_range;
  if (n_big) *n_big = (uint32_t)scene->n_big;
  if (big_r) memcpy(big_r, scene->big_r, sizeof scene->big_r);
  if (big_c) memcpy(big_c, scene->big_c, sizeof scene->big_c);
  return RT_HIP_OK;
}

int rt_hip_scene_update_vertices(RtHipScene *scene, const double *d_positions, size_t n_triangles)
{
  return guarded("rt_hip_scene_update_vertices", [&] { return scene_update_impl(scene, d_positions, n_triangles, false); });
}

int rt_hip_scene_update_vertices_host(RtHipScene *scene, const double *h_positions, size_t n_triangles)
{
  return guarded("rt_hip_scene_update_vertices_host", [&] { return scene_update_impl(scene, h_positions, n_triangles, true); });
}

int rt_hip_scene_update_info(const RtHipScene *scene, uint64_t *updates, double *last_seconds)
{
  if (!scene)
    return fail(RT_HIP_EINVAL, "rt_hip_scene_update_info: scene is NULL");
  if (updates) *updates = scene->updates;
  if (last_seconds) *last_seconds = scene->last_update_seconds;
  return RT_HIP_OK;
}

int rt_hip_scene_read_triangles(const RtHipScene *scene, double *geom, double *normal, double *entry, uint32_t *object)
{
  if (!scene)
    return fail(RT_HIP_EINVAL, "rt_hip_scene_read_triangles: scene is NULL");
  const size_t n = scene->view.n_triangles;
  if (n == 0)
    return RT_HIP_OK;
  DeviceScope on(scene->device);
  HIP_TRY(on.status);
  if (geom) HIP_TRY(hipMemcpy(geom, scene->view.tri_geom, 72 * n, hipMemcpyDeviceToHost));
  if (normal) HIP_TRY(hipMemcpy(normal, scene->view.tri_normal, 24 * n, hipMemcpyDeviceToHost));
  if (entry)
    HIP_TRY(hipMemcpy(entry, scene->view.entry_src + PT_ENTRY_SRC_STRIDE * (size_t)scene->view.n_spheres, PT_ENTRY_SRC_STRIDE * 8 * n,
                      hipMemcpyDeviceToHost));
  if (object) HIP_TRY(hipMemcpy(object, scene->view.tri_object, 4 * n, hipMemcpyDeviceToHost));
  return RT_HIP_OK;
}

int rt_hip_scene_bounds(const RtHipScene *scene, double mesh_center[3], double *mesh_radius, double *reach, uint32_t *mesh_round)
{
  if (!scene)
    return fail(RT_HIP_EINVAL, "rt_hip_scene_bounds: scene is NULL");
  if (mesh_center) memcpy(mesh_center, scene->mesh_c, sizeof scene->mesh_c);
  if (mesh_radius) *mesh_radius = scene->mesh_R;
  if (reach) *reach = scene->reach;
  if (mesh_round) *mesh_round = scene->view.mesh_round;
  return RT_HIP_OK;
}

const char *rt_hip_kernel_name(const RtHipScene *scene, uint32_t integrator)
{
  if (!scene)
    return "";
  /* a scene whose parked-walk workspace could not be allocated runs on the lane-waiting kernels: report what a launch
   * takes, so that an out-of-memory fallback cannot pass as a measurement of the parked-walk kernels.  What is assumed of
   * the launch itself: sums that fit (one sample at depth 0, one chunk), a pending-ray pool of full width --
   * rt_hip_last_launch_kernel() has the fact. */
  PtPlanAsk ask = ask_for(scene, integrator, 1, 0, 1, false, 0, park_ws_expected(scene));
  ask.wide_pend_ok = !(g_fail_alloc.load() & RT_HIP_FAIL_ALLOC_WIDE_PEND);
  return pt_kernel_name_of(pt_plan_launch(scene->view, ask).kernel);
}

const char *rt_hip_last_launch_kernel(void) { return pt_kernel_name_of(g_last_kernel); }

int rt_hip_kernel_count(void) { return pt_kernel_count(); }

const char *rt_hip_kernel_launches(int index, uint64_t *launches)
{
  return kernel_launches_of(index, launches, pt_kernel_count(), pt_kernel_name_of, pt_kernel_launches);
}

const char *rt_hip_kernel_for_class(const RtHipSceneClass *c)
{
  if (!c)
    return "";
  PtSceneView v;
  memset(&v, 0, sizeof v);
  v.n_spheres = c->n_spheres;
  v.n_meshes = c->n_meshes;
  v.n_triangles = c->n_triangles;
  v.n_bvh_nodes = c->n_triangles ? std::max(1u, c->n_triangles / 8u) : 0u;
  v.any_checker = c->any_checker ? 1u : 0u;
  v.any_refract = c->any_refract ? 1u : 0u;
  v.any_mirror_glass = c->any_mirror_glass ? 1u : 0u;
  v.wide_range = c->wide_range ? 1u : 0u;
  v.mesh_round = c->mesh_round ? 1u : 0u;
  /* one chunk of samples_per_chunk samples, without a chunk workspace: the class's facts go to the pick unchanged */
  const PtPlanAsk ask = {.integrator = c->integrator, .samples = c->samples_per_chunk, .max_depth = c->max_depth, .max_emission = c->max_emission,
                         .sample_chunks = 1, .have_park_ws = c->have_park_ws != 0, .wide_pend_ok = c->wide_pend_ok != 0};
  return pt_kernel_name_of(pt_plan_launch(v, ask).kernel);
}

void rt_hip_selftest_fail_alloc(uint32_t mask) { g_fail_alloc.store(mask); }

uint64_t rt_hip_mixed_grid_launches(void) { return g_mixed_launches.load(); }

int rt_hip_selftest_pool_slots(int device, uint32_t *park_slots_per_xcd, uint32_t *pend_slots_per_xcd)
{
  if (!have_device(device))
    return fail(RT_HIP_ENODEV, "no HIP device %d", device);
  DeviceScope scope(device);
  HIP_TRY(scope.status);
  if (park_slots_per_xcd)
    *park_slots_per_xcd = pt_pool_slots_per_xcd(true);
  if (pend_slots_per_xcd)
    *pend_slots_per_xcd = pt_pool_slots_per_xcd(false);
  return RT_HIP_OK;
}

int rt_hip_pool_bytes(int device, size_t *park_ws_bytes, size_t *pend_pool_bytes)
{
  if (device < 0 || device >= 64 || device >= usable_devices())
    return fail(RT_HIP_ENODEV, "no HIP device %d", device);
  if (park_ws_bytes)
  {
    std::lock_guard<std::mutex> lock(g_park_mutex);
    const ParkPool &p = g_park[device];
    *park_ws_bytes = p.ws ? park_flag_bytes(p.slots_per_xcd) + (size_t)PT_PARK_XCDS * p.slots_per_xcd * (PT_BLOCK / 64) * (size_t)PT_PARK_WAVE_BYTES : 0;
  }
  if (pend_pool_bytes)
  {
    std::lock_guard<std::mutex> lock(g_pend_mutex);
    const PendPool &p = g_pend[device];
    *pend_pool_bytes = p.ws ? pend_flag_bytes(p.slots_per_xcd) + (size_t)PT_PARK_XCDS * p.slots_per_xcd * p.entries * PT_PEND_FIELDS_HOST * p.columns * sizeof(double) : 0;
  }
  return RT_HIP_OK;
}

int rt_hip_launch_status(int device, uint32_t *flags)
{
  uint32_t f = 0;
  if (flags)
    *flags = 0;
  if (!have_device(device))
    return fail(RT_HIP_ENODEV, "no HIP device %d", device);
  DeviceScope scope(device);
  HIP_TRY(scope.status);
  int rc = status_take(device, &f);
  if (rc)
    return rc;
  if (flags)
    *flags = f;
  return status_to_error(f);
}

size_t rt_hip_chunk_workspace_bytes(uint32_t tile_count)
{ /* enough for any scene: the windowed sums of the M_REFRACTION forms are the larger record */
  return (size_t)tile_count * PT_ACC_WS_WORDS_WIN * sizeof(unsigned long long);
}

size_t rt_hip_scene_chunk_workspace_bytes(const RtHipScene *scene, uint32_t tile_count)
{
  const bool windowed = !scene || scene->view.any_refract;
  return (size_t)tile_count * (windowed ? PT_ACC_WS_WORDS_WIN : PT_ACC_WS_WORDS) * sizeof(unsigned long long);
}

uint32_t rt_hip_suggest_chunks(const RtHipScene *scene, uint32_t tile_count, int32_t samples)
{
  return rt_hip_suggest_chunks_depth(scene, tile_count, samples, 0);
}

uint32_t rt_hip_suggest_chunks_depth(const RtHipScene *scene, uint32_t tile_count, int32_t samples, int32_t max_depth)
{
  if (!scene || tile_count == 0 || samples < 1)
    return 1;
  /* scenes with M_REFRACTION: at least as many chunks as the windowed sums need (pt_refr_pool_fits per chunk) */
  const uint64_t need = pt_refr_chunk_floor(scene->view, samples, max_depth, tile_count);
  if (samples < 128)
    return (uint32_t)need;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, scene->device) != hipSuccess)
    return (uint32_t)need;
  /* which body the scene takes (the plan of a launch with a chunk workspace): the parked-walk kernels render a tile per WAVE
   * (four per workgroup, four workgroups per CU), and a chunk of theirs must be longer -- a wave amortises its walk batches and
   * its final, partly filled walk over its pool */
  const PtPlan plan =
      pt_plan_launch(scene->view, ask_for(scene, RT_HIP_TRACE_PATH, samples, max_depth, 1, true, tile_count, park_ws_expected(scene)));
  uint64_t want, min_chunk_samples;
  if (plan.queued)
  {
    /* >= 30 rounds of workgroups (the expensive tiles -- those on the mesh -- are few and long: one workgroup of four of them at
     * 4096 spp outlasts a rank's whole ideal share at N = 8), >= 128 samples per chunk.  One rank's share of config 5 at N = 8,
     * ms by chunks (tools/shard_chunks.py, profiles/r05_shard_chunks.txt): 4096 spp 1: 608, 2: 505, 4: 465, 8: 447, 12: 443, 16: 443
     * (ideal 418); 256 spp 1: 39.2, 2: 37.1, 4: 41.8, 8: 42.6 (ideal 27.0).  Round 4's rule (tiles, not workgroups; 64 samples)
     * gave 2 and 4. */
    want = 30ull * 4ull * 4ull * (uint64_t)prop.multiProcessorCount;
  }
  else
  {
    /* aim for >= 20 workgroups per resident slot (5 per CU), so the last, partly filled round
     * of the launch is a small fraction of it.  (One rank's share of the headline frame at
     * N = 8 / 4 / 2, ms by chunks: 2: 30.0, 4: 29.3, 6: 29.4, 8: 29.6, 16: 30.9 / 1: 59.1, 2: 57.7, 4: 57.5 / 1: 114.7, 2: 113.4.) */
    want = 20ull * 5ull * (uint64_t)prop.multiProcessorCount;
  }
  /* a chunk keeps >= 128 samples (a workgroup's fixed costs -- staging, keys, culling, the resolve pass -- against its pool: config 3's
   * share at N = 8, 256 spp, ms by chunks 1: 2.63, 2: 2.61, 4: 2.70, 8: 3.01); the M_REFRACTION forms >= 64 (a refractive sample
   * is two to three times the rays: the glass mesh's share at N = 8, 256 spp 2: 48.8, 4: 45.9, 8: 46.9) */
  min_chunk_samples = plan.windowed ? 64 : 128;
  uint64_t chunks = (want + tile_count - 1) / tile_count;
  const uint64_t cap = (uint64_t)samples / min_chunk_samples;
  if (chunks > cap) chunks = cap;
  if (chunks > 16) chunks = 16;
  if (chunks < need) chunks = need;
  return chunks < 1 ? 1u : (uint32_t)chunks;
}

int rt_hip_render_tiles(const RtHipScene *scene, const RtHipCamera *camera, const RtHipParams *params,
                        float *d_tiles_rgb, uint8_t *d_tiles_rgb8, uint64_t *d_stats, void *stream)
{
  return rt_hip_render_tiles_chunked(scene, camera, params, 1, nullptr, d_tiles_rgb, d_tiles_rgb8, d_stats, stream);
}

int rt_hip_render_tiles_chunked(const RtHipScene *scene, const RtHipCamera *camera, const RtHipParams *params,
                                uint32_t sample_chunks, void *d_workspace, float *d_tiles_rgb,
                                uint8_t *d_tiles_rgb8, uint64_t *d_stats, void *stream)
{
  if (!scene || !camera || !d_tiles_rgb)
    return fail(RT_HIP_EINVAL, "scene, camera and d_tiles_rgb are required");
  if (sample_chunks < 1 || (params && (int64_t)sample_chunks > params->samples))
    return fail(RT_HIP_EINVAL, "sample_chunks must be in [1, samples]");
  if (sample_chunks > 1 && !d_workspace)
    return fail(RT_HIP_EINVAL, "sample_chunks > 1 needs a workspace of rt_hip_chunk_workspace_bytes(tile_count)");
  return guarded("rt_hip_render_tiles_chunked", [&]() -> int {
    PtLaunch L;
    bool empty = false;
    int rc = launch_prepare(scene, camera, params, L, &empty);
    if (rc || empty)
      return rc;
    L.acc_ws = static_cast<unsigned long long *>(d_workspace);
    L.tiles_rgb = d_tiles_rgb;
    L.tiles_rgb8 = d_tiles_rgb8;
    L.stats = reinterpret_cast<unsigned long long *>(d_stats);
    DeviceScope scope(scene->device);
    HIP_TRY(scope.status);
    rc = launch_device_state(scene, L);
    if (rc)
      return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    size_t slot = 0;
    rc = acquire_tables(scene, L.near_R, st, &L.scene.filt, &L.scene.bvh_nodes, &slot);
    if (rc)
      return rc;
    /* the device's pending-ray pool, where the plan needs one: g_pend_mutex from the lookup until the launch is enqueued */
    std::unique_lock<std::mutex> pend_lock(g_pend_mutex, std::defer_lock);
    PtPlan plan;
    rc = plan_launch(scene, L, sample_chunks, d_workspace != nullptr,
                     [&](uint32_t entries, uint32_t columns, PtLaunch &launch) {
                       if (!pend_lock.owns_lock())
                         pend_lock.lock();
                       return pend_pool_for(scene->device, entries, columns, launch);
                     },
                     &plan);
    if (!rc && (uint64_t)L.tile_count * L.sample_chunks > 0x7FFFFFFFull)
      rc = fail(RT_HIP_EINVAL, "tile_count x sample_chunks exceeds the grid limit");
    /* one chunk asked and no workspace given: the mixed grid, where the rule takes it and its workspace can be had */
    std::unique_lock<std::mutex> tail_lock(g_tail_mutex, std::defer_lock);
    uint32_t n_whole = 0, tail_chunks = 0;
    if (!rc && sample_chunks == 1 && !d_workspace && grid_split_for(L, plan, scene->device, &n_whole, &tail_chunks))
    {
      tail_lock.lock();
      if (unsigned long long *ws = grid_tail_ws(scene->device, L.tile_count - n_whole, st))
      {
        L.acc_ws = ws;
        L.n_whole = n_whole;
        L.sample_chunks = tail_chunks;
      }
      else
        tail_lock.unlock();
    }
    const hipError_t e = rc ? hipSuccess : pt_launch_render(L, st, plan.kernel);
    if (tail_lock.owns_lock())
    {
      grid_tail_used(scene->device, st);
      if (e == hipSuccess && L.n_whole != 0u)
        g_mixed_launches.fetch_add(1);
      tail_lock.unlock();
    }
    if (pend_lock.owns_lock())
      pend_lock.unlock();
    release_tables(scene, slot, st);
    if (!rc)
      rc = launched(e, pt_kernel_name_of(plan.kernel));
    if (!rc)
      g_last_kernel = plan.kernel;
    return rc;
  });
}

/* ---- progressive rendering: one frame accumulated over passes (RtHipAccum, above) ---- */

int rt_hip_accum_create(const RtHipScene *scene, const RtHipCamera *camera, const RtHipParams *params, RtHipAccum **out)
{
  if (out)
    *out = nullptr;
  if (!scene || !camera || !params || !out)
    return fail(RT_HIP_EINVAL, "scene, camera, params and out are required");
  if (params->samples < 1)
    return fail(RT_HIP_EINVAL, "the sample budget (params->samples) must be >= 1");
  return guarded("rt_hip_accum_create", [&]() -> int {
    PtLaunch L;
    bool empty = false;
    int rc = launch_prepare(scene, camera, params, L, &empty);
    if (rc)
      return rc;
    if (empty)
      return fail(RT_HIP_EINVAL, "an accumulation needs tile_count >= 1");
    DeviceScope scope(scene->device);
    HIP_TRY(scope.status);
    rc = launch_device_state(scene, L);
    if (rc)
      return rc;
    RtHipAccum *a = new (std::nothrow) RtHipAccum();
    if (!a)
      return fail(RT_HIP_ENOMEM, "accumulation: out of host memory");
    a->scene = scene;
    scene->live_accums++; /* until accum_free: the plan below holds the scene's view, so its vertices may not move meanwhile */
    /* the plan of a one-shot launch of the whole budget with a chunk workspace and the suggested chunks: the same member, the same
     * sum form, the same fallback rows; the fixed-point scale is the budget's (launch_prepare) */
    const uint32_t chunks = rt_hip_suggest_chunks_depth(scene, params->tile_count, params->samples, params->max_depth);
    PtPlan plan;
    rc = plan_launch(scene, L, chunks, true,
                     [&](uint32_t entries, uint32_t columns, PtLaunch &launch) { return pend_pool_own(entries, columns, launch, a->pend); }, &plan);
    if (!rc && plan.kernel < 0)
      rc = fail(RT_HIP_ERUNTIME, "no kernel for this scene"); /* unreachable (pt_pick_kernel) */
    if (rc)
    {
      accum_free(a);
      return rc;
    }
    a->kernel = plan.kernel;
    a->takes_chunks = pt_kernel_takes_chunks(plan.kernel);
    a->budget = params->samples;
    a->plan_spc = (int32_t)(((int64_t)params->samples + plan.sample_chunks - 1) / plan.sample_chunks);
    L.acc_keep = 1u;
    const size_t bytes = a->takes_chunks ? (size_t)L.tile_count * (plan.windowed ? PT_ACC_WS_WORDS_WIN : PT_ACC_WS_WORDS) * sizeof(unsigned long long)
                                         : (size_t)L.tile_count * 3u * PT_BLOCK * sizeof(double);
    hipError_t e = a->sums.alloc(bytes);
    if (e != hipSuccess)
    {
      accum_free(a);
      return fail(RT_HIP_ENOMEM, "accumulation sums (%zu MB): %s", bytes >> 20, hipGetErrorString(e));
    }
    e = hipMemset(a->sums.ptr, 0, bytes);
    if (e == hipSuccess)
      e = hipStreamSynchronize(nullptr); /* zero before a pass on any stream adds to them */
    if (e != hipSuccess)
    {
      (void)hipGetLastError();
      accum_free(a);
      return fail(RT_HIP_ERUNTIME, "accumulation sums: %s", hipGetErrorString(e));
    }
    if (a->takes_chunks)
      L.acc_ws = a->sums.at<unsigned long long>();
    else
      L.slice_ws = a->sums.at<double>();
    a->L = L;
    *out = a;
    return RT_HIP_OK;
  });
}

int rt_hip_accum_add(RtHipAccum *a, int32_t samples, uint64_t *d_stats, void *stream)
{
  if (!a)
    return fail(RT_HIP_EINVAL, "accumulation is NULL");
  if (samples <= 0 || samples > a->budget - a->done)
    return fail(RT_HIP_EINVAL, "a pass takes 1 .. %d samples (budget %d, %d done), not %d", a->budget - a->done, a->budget, a->done, samples);
  if (a->broken)
    return fail(RT_HIP_ERUNTIME, "the accumulation is unusable: an earlier freeze failed on the device");
  return guarded("rt_hip_accum_add", [&]() -> int {
    const RtHipScene *scene = a->scene;
    PtLaunch L = a->L;
    L.samples = samples;
    L.sample_first = (uint32_t)a->done;
    L.stats = reinterpret_cast<unsigned long long *>(d_stats);
    L.sample_chunks = 1u;
    /* with frozen tiles the pass renders the live slots only, and the chunks are planned for that many tiles */
    const uint32_t pass_tiles = a->any_frozen ? a->live_count : L.tile_count;
    if (pass_tiles == 0u)
      return RT_HIP_OK; /* every tile is frozen: nothing is rendered and `done` stays */
    if (a->any_frozen)
    {
      L.slot_list = a->slot_list;
      L.slot_count = a->live_count;
    }
    if (a->takes_chunks)
    { /* no workgroup gets more samples than the plan's chunks have (that is what the windowed words are sized by), and a small
       * tile count gets the chunks the suggestion asks for.  Capacity: every chunk adds at most one piece below 2^32 to a word of
       * the tile records, and every chunk has at least one sample, so over all passes a word takes at most budget < 2^31 pieces */
      uint64_t chunks = ((uint64_t)samples + (uint64_t)a->plan_spc - 1u) / (uint64_t)a->plan_spc;
      chunks = std::max<uint64_t>(chunks, rt_hip_suggest_chunks_depth(scene, pass_tiles, samples, L.max_depth));
      chunks = std::min<uint64_t>(chunks, (uint64_t)samples);
      if ((uint64_t)pass_tiles * chunks > 0x7FFFFFFFull)
        return fail(RT_HIP_EINVAL, "tile_count x sample_chunks exceeds the grid limit");
      L.sample_chunks = (uint32_t)chunks;
    }
    DeviceScope scope(scene->device);
    HIP_TRY(scope.status);
    size_t slot = 0;
    int rc = acquire_tables(scene, L.near_R, static_cast<hipStream_t>(stream), &L.scene.filt, &L.scene.bvh_nodes, &slot);
    if (rc)
      return rc;
    const hipError_t e = pt_launch_render(L, static_cast<hipStream_t>(stream), a->kernel);
    release_tables(scene, slot, static_cast<hipStream_t>(stream));
    if (e != hipSuccess)
      return fail(RT_HIP_ERUNTIME, "%s pass: %s", pt_kernel_name_of(a->kernel), hipGetErrorString(e));
    a->done += samples;
    return RT_HIP_OK;
  });
}

int rt_hip_accum_add_host(RtHipAccum *a, int32_t samples, uint64_t *h_stats, double *kernel_seconds)
{
  if (kernel_seconds)
    *kernel_seconds = 0;
  if (!a)
    return fail(RT_HIP_EINVAL, "accumulation is NULL");
  DeviceScope scope(a->scene->device);
  HIP_TRY(scope.status);
  DeviceBuffer d_stats;
  EventPair timer;
  HIP_TRY(d_stats.alloc(RT_HIP_NSTATS * sizeof(uint64_t)));
  HIP_TRY(hipMemset(d_stats.ptr, 0, RT_HIP_NSTATS * sizeof(uint64_t)));
  HIP_TRY(timer.create());
  HIP_TRY(timer.start(nullptr));
  const int rc = rt_hip_accum_add(a, samples, d_stats.at<uint64_t>(), nullptr);
  if (rc)
    return rc;
  HIP_TRY(timer.stop(nullptr));
  HIP_TRY(timer.wait());
  uint64_t st[RT_HIP_NSTATS] = {0, 0, 0, 0};
  HIP_TRY(hipMemcpy(st, d_stats.ptr, sizeof st, hipMemcpyDeviceToHost));
  float ms = 0.f;
  HIP_TRY(timer.elapsed_ms(&ms));
  if (h_stats)
    for (int k = 0; k < RT_HIP_NSTATS; k++)
      h_stats[k] += st[k];
  if (kernel_seconds)
    *kernel_seconds = 1e-3 * (double)ms;
  return RT_HIP_OK;
}

int rt_hip_accum_resolve(const RtHipAccum *a, float *d_tiles_rgb, uint8_t *d_tiles_rgb8, void *stream)
{
  if (!a || !d_tiles_rgb)
    return fail(RT_HIP_EINVAL, "accumulation and d_tiles_rgb are required");
  if (a->done < 1)
    return fail(RT_HIP_EINVAL, "the accumulation holds no sample yet");
  if (a->broken)
    return fail(RT_HIP_ERUNTIME, "the accumulation is unusable: an earlier freeze failed on the device");
  PtLaunch L = a->L;
  L.samples = a->done;
  L.tiles_rgb = d_tiles_rgb;
  L.tiles_rgb8 = d_tiles_rgb8;
  DeviceScope scope(a->scene->device);
  HIP_TRY(scope.status);
  const hipError_t e = pt_launch_resolve(L, a->any_frozen ? a->tile_samples.at<uint32_t>() : nullptr, static_cast<hipStream_t>(stream), a->kernel);
  if (e != hipSuccess)
    return fail(RT_HIP_ERUNTIME, "accumulation resolve: %s", hipGetErrorString(e));
  return RT_HIP_OK;
}

int rt_hip_accum_read_image(const RtHipAccum *a, float *h_rgb, uint8_t *h_rgb8)
{
  if (!a || (!h_rgb && !h_rgb8))
    return fail(RT_HIP_EINVAL, "accumulation and an output are required");
  const PtLaunch &L = a->L;
  const size_t tile_vals = (size_t)L.tile_count * PT_TILE_PIXELS * 3, img_vals = (size_t)L.width * L.height * 3;
  DeviceScope scope(a->scene->device);
  HIP_TRY(scope.status);
  HIP_TRY(hipDeviceSynchronize()); /* the passes, on whatever stream they ran */
  DeviceBuffer buf;                /* tiles f32 + u8, image f32 + u8 */
  HIP_TRY(buf.alloc(tile_vals * 5 + img_vals * 5));
  float *tiles = buf.at<float>(0), *img = buf.at<float>(tile_vals * 5);
  uint8_t *tiles8 = buf.at<uint8_t>(tile_vals * 4), *img8 = buf.at<uint8_t>(tile_vals * 5 + img_vals * 4);
  int rc = rt_hip_accum_resolve(a, tiles, tiles8, nullptr);
  if (rc)
    return rc;
  HIP_TRY(hipMemset(img, 0, img_vals * 5));
  HIP_TRY(pt_launch_untile(tiles, tiles8, L.width, L.height, L.tile_first, L.tile_stride, L.tile_count, img, img8, nullptr));
  if (h_rgb)
    HIP_TRY(hipMemcpy(h_rgb, img, img_vals * sizeof(float), hipMemcpyDeviceToHost));
  if (h_rgb8)
    HIP_TRY(hipMemcpy(h_rgb8, img8, img_vals, hipMemcpyDeviceToHost));
  uint32_t flags = 0;
  rc = status_take(a->scene->device, &flags);
  return rc ? rc : status_to_error(flags);
}

int32_t rt_hip_accum_samples(const RtHipAccum *a) { return a ? a->done : 0; }

const char *rt_hip_accum_kernel(const RtHipAccum *a) { return a ? pt_kernel_name_of(a->kernel) : ""; }

void rt_hip_accum_destroy(RtHipAccum *a) { accum_free(a); }

/* ---- adaptive sampling: the error estimate, the freeze, the driver (rt_hip.h) ------------------------------------------------ */

int rt_hip_tile_error(const float *d_cur, const float *d_prev, int32_t width, int32_t height, uint32_t tile_first, uint32_t tile_stride,
                      uint32_t tile_count, float *d_error, void *stream)
{
  if (!d_cur || !d_prev || !d_error)
    return fail(RT_HIP_EINVAL, "d_cur, d_prev and d_error are required");
  if (width < 1 || height < 1)
    return fail(RT_HIP_EINVAL, "width and height must be >= 1");
  if (tile_count == 0)
    return RT_HIP_OK;
  if (tile_stride == 0 && tile_count > 1)
    return fail(RT_HIP_EINVAL, "tile_stride must be >= 1");
  const uint64_t n_tiles = (uint64_t)tiles_x_of(width) * tiles_y_of(height);
  if ((uint64_t)tile_first + (uint64_t)(tile_count - 1) * tile_stride >= n_tiles)
    return fail(RT_HIP_EINVAL, "tile range outside the image");
  int on = -1;
  for (const void *ptr : {static_cast<const void *>(d_cur), static_cast<const void *>(d_prev), static_cast<const void *>(d_error)})
  {
    int device = -1;
    const int rc = device_of(ptr, "one of d_cur, d_prev and d_error", &device);
    if (rc)
      return rc;
    if (on >= 0 && device != on)
      return fail(RT_HIP_EINVAL, "d_cur, d_prev and d_error must be on one device (%d, %d)", on, device);
    on = device;
  }
  DeviceScope scope(on);
  HIP_TRY(scope.status);
  const hipError_t e = pt_launch_tile_error(d_cur, d_prev, width, height, tile_first, tile_stride, tile_count, d_error, static_cast<hipStream_t>(stream));
  if (e != hipSuccess)
    return fail(RT_HIP_ERUNTIME, "tile error: %s", hipGetErrorString(e));
  return RT_HIP_OK;
}

int rt_hip_accum_freeze(RtHipAccum *a, const float *d_error, double threshold, uint32_t dilate, uint32_t *live_count, void *stream)
{
  if (a && !d_error)
    return fail(RT_HIP_EINVAL, "d_error is required (rt_hip_accum_freeze_mask takes a host mask)");
  return accum_freeze(a, d_error, nullptr, threshold, dilate, live_count, stream);
}

int rt_hip_accum_freeze_mask(RtHipAccum *a, const uint8_t *h_keep, uint32_t *live_count, void *stream)
{
  if (a && !h_keep)
    return fail(RT_HIP_EINVAL, "h_keep is required");
  return accum_freeze(a, nullptr, h_keep, 0.0, 0u, live_count, stream);
}

int rt_hip_accum_tile_samples(const RtHipAccum *a, uint32_t *h_counts)
{
  if (!a || !h_counts)
    return fail(RT_HIP_EINVAL, "accumulation and h_counts are required");
  const uint32_t n = a->L.tile_count;
  if (a->tile_samples)
  {
    DeviceScope scope(a->scene->device);
    HIP_TRY(scope.status);
    /* a freeze has waited for its stream before it returned: the counts are at rest, and a copy on the null stream is enough */
    HIP_TRY(hipMemcpy(h_counts, a->tile_samples.ptr, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost));
  }
  for (uint32_t k = 0; k < n; k++)
    if (!a->tile_samples || h_counts[k] == 0u)
      h_counts[k] = (uint32_t)a->done; /* a live slot holds every sample done so far */
  return RT_HIP_OK;
}

uint32_t rt_hip_accum_live_tiles(const RtHipAccum *a) { return !a ? 0u : (a->tile_samples ? a->live_count : a->L.tile_count); }

void rt_hip_adapt_defaults(RtHipAdaptParams *p)
{
  if (!p)
    return;
  p->min_samples = 16;
  p->dilate = 1u;
  p->threshold = 0.02;
}

int rt_hip_adapt_schedule(int32_t budget, int32_t min_samples, int32_t *targets, int32_t cap)
{
  if (budget < 1 || min_samples < 1)
    return 0;
  int n = 0;
  const int64_t h = std::max<int64_t>(1, min_samples / 2);
  for (int64_t t = h;; t *= 2)
  {
    const int32_t target = (int32_t)std::min<int64_t>(t, budget);
    if (targets && n < cap)
      targets[n] = target;
    n++;
    if (target == budget)
      break;
  }
  return n;
}

int rt_hip_accum_run_adaptive(RtHipAccum *a, const RtHipAdaptParams *p, uint64_t *h_stats, double *kernel_seconds,
                              int (*on_checkpoint)(void *user, int32_t samples_done, uint32_t live_tiles), void *user)
{
  if (kernel_seconds)
    *kernel_seconds = 0;
  if (!a || !p)
    return fail(RT_HIP_EINVAL, "accumulation and params are required");
  int rc = check_adapt(p);
  if (rc)
    return rc;
  if (a->done != 0)
    return fail(RT_HIP_EINVAL, "the driver starts from an empty accumulation (%d samples done)", a->done);
  DeviceScope scope(a->scene->device);
  HIP_TRY(scope.status);
  double seconds = 0;
  rc = adaptive_passes(a, p, h_stats, on_checkpoint, user, &seconds);
  if (kernel_seconds)
    *kernel_seconds = seconds;
  return rc;
}

int rt_hip_selftest_math(int op, const double *h_a, const double *h_b, double *h_out, size_t n, int device)
{
  if (!h_a || !h_b || !h_out || op < 0 || op > 9 || (op == 8 && n < 8) || (op == 9 && n % 8 != 0))
    return fail(RT_HIP_EINVAL, "bad self-test arguments");
  if (!have_device(device))
    return fail(RT_HIP_ENODEV, "no HIP device %d", device);
  if (n == 0)
    return RT_HIP_OK;
  DeviceScope scope(device);
  HIP_TRY(scope.status);
  DeviceBuffer buf;
  HIP_TRY(buf.alloc(3 * n * sizeof(double)));
  double *d = buf.at<double>();
  HIP_TRY(hipMemcpy(d, h_a, n * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d + n, h_b, n * sizeof(double), hipMemcpyHostToDevice));
  /* op 8 accumulates into out, starting from what the caller put there */
  HIP_TRY(op == 8 ? hipMemcpy(d + 2 * n, h_out, n * sizeof(double), hipMemcpyHostToDevice) : hipMemset(d + 2 * n, 0, n * sizeof(double)));
  HIP_TRY(pt_launch_selftest(op, d, d + n, d + 2 * n, n, nullptr));
  HIP_TRY(hipMemcpy(h_out, d + 2 * n, n * sizeof(double), hipMemcpyDeviceToHost));
  return RT_HIP_OK;
}

int rt_hip_selftest_xcc(uint32_t n_workgroups, uint32_t h_counts[16], int device)
{
  if (!h_counts || n_workgroups == 0 || n_workgroups > (1u << 20))
    return fail(RT_HIP_EINVAL, "bad self-test arguments");
  if (!have_device(device))
    return fail(RT_HIP_ENODEV, "no HIP device %d", device);
  DeviceScope scope(device);
  HIP_TRY(scope.status);
  DeviceBuffer buf;
  HIP_TRY(buf.alloc(16 * sizeof(unsigned int)));
  HIP_TRY(hipMemset(buf.ptr, 0, 16 * sizeof(unsigned int)));
  HIP_TRY(pt_launch_selftest_xcc(buf.at<unsigned int>(), n_workgroups, nullptr));
  HIP_TRY(hipMemcpy(h_counts, buf.ptr, 16 * sizeof(unsigned int), hipMemcpyDeviceToHost));
  return RT_HIP_OK;
}

int rt_hip_selftest_intersect(int kind, const double *h_rays, const double *h_prims, size_t n, double near_R,
                              uint8_t *h_hit, double *h_tuv, uint64_t *h_keep, int device)
{
  if ((kind != 0 && kind != 1 && kind != 2) || !h_rays || !h_prims || !h_hit || !h_tuv || !h_keep)
    return fail(RT_HIP_EINVAL, "bad self-test arguments");
  if (!(near_R > 0) || !(near_R < 1e15) || n > 0x7FFFFFFFu)
    return fail(RT_HIP_EINVAL, "near_R must be a positive finite bound, n < 2^31");
  if (!have_device(device))
    return fail(RT_HIP_ENODEV, "no HIP device %d", device);
  if (kind == 2 && n % 64 != 0)
    return fail(RT_HIP_EINVAL, "the matrix-filter self-test takes whole blocks of 64 cases");
  if (n == 0)
    return RT_HIP_OK;
  return guarded("rt_hip_selftest_intersect", [&]() -> int {
    /* the records exactly as rt_hip_scene_create lays them out (same helpers) */
    const size_t rec = kind == 1 ? 9 : 4;
    std::vector<double> prims(rec * n), entry(PT_ENTRY_SRC_STRIDE * n);
    double max_center = 0;
    for (size_t i = 0; i < n; i++)
    {
      double *e = &entry[PT_ENTRY_SRC_STRIDE * i];
      if (kind != 1)
      {
        const double *p = h_prims + 4 * i;
        if (!(std::fabs(p[3]) >= 1e-100) || !(std::fabs(p[3]) <= 1e17))
          return fail(RT_HIP_ELIMIT, "sphere %zu: |radius| %g outside [1e-100, 1e17]", i, p[3]);
        scene_sphere_entry(p, p[3], e, nullptr);
        memcpy(&prims[4 * i], e, 4 * sizeof(double));
      }
      else
        scene_triangle_entry(h_prims + 9 * i, h_prims + 9 * i + 3, h_prims + 9 * i + 6, &prims[9 * i], e);
      if (!(e[4] <= 1e17))
        return fail(RT_HIP_ELIMIT, "primitive %zu: centre beyond 1e17", i);
      max_center = std::fmax(max_center, e[4]);
    }
    const double filt_shift = 12.0 * 5.9604644775390625e-08 * (max_center + near_R) * (1.0 + 1e-9); /* as rt_hip_render_tiles */
    const size_t n_blocks = (n + 63) / 64;
    const size_t filt_bytes = (n_blocks * 32 + 1) * (size_t)PT_FILT_STRIDE * 2 * sizeof(float);
    const size_t b_rays = 6 * n * 8, b_prims = rec * n * 8, b_entry = entry.size() * 8, b_tuv = 3 * n * 8, b_keep = 3 * n * 8;
    auto pad = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t b_tri32 = kind == 1 ? n * PT_TRI32_STRIDE * sizeof(float) : 0;
    const size_t o_rays = 0, o_prims = o_rays + pad(b_rays), o_entry = o_prims + pad(b_prims), o_filt = o_entry + pad(b_entry),
                 o_tri32 = o_filt + pad(filt_bytes), o_tuv = o_tri32 + pad(b_tri32), o_keep = o_tuv + pad(b_tuv),
                 o_hit = o_keep + pad(b_keep), total = o_hit + pad(n);
    DeviceScope scope(device);
    HIP_TRY(scope.status);
    DeviceBuffer d;
    const hipError_t e = d.alloc(total);
    if (e != hipSuccess)
      return fail(RT_HIP_ENOMEM, "hipMalloc(%zu): %s", total, hipGetErrorString(e));
    HIP_TRY(hipMemset(d.at<char>(o_filt), 0, filt_bytes));
    HIP_TRY(hipMemcpy(d.at<char>(o_rays), h_rays, b_rays, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d.at<char>(o_prims), prims.data(), b_prims, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d.at<char>(o_entry), entry.data(), b_entry, hipMemcpyHostToDevice));
    HIP_TRY(pt_launch_selftest_intersect(kind, d.at<double>(o_rays), d.at<double>(o_prims), d.at<double>(o_entry), d.at<float>(o_filt),
                                         d.at<float>(o_tri32), (uint32_t)n, near_R, filt_shift, d.at<uint8_t>(o_hit), d.at<double>(o_tuv),
                                         d.at<unsigned long long>(o_keep), nullptr));
    HIP_TRY(hipMemcpy(h_hit, d.at<char>(o_hit), n, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(h_tuv, d.at<char>(o_tuv), b_tuv, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(h_keep, d.at<char>(o_keep), b_keep, hipMemcpyDeviceToHost));
    return RT_HIP_OK;
  });
}

int rt_hip_untile(const float *d_tiles_rgb, const uint8_t *d_tiles_rgb8, int32_t width, int32_t height,
                  uint32_t tile_first, uint32_t tile_stride, uint32_t tile_count, float *d_image_rgb,
                  uint8_t *d_image_rgb8, void *stream)
{
  if (width < 1 || height < 1)
    return fail(RT_HIP_EINVAL, "bad image size");
  if ((d_image_rgb && !d_tiles_rgb) || (d_image_rgb8 && !d_tiles_rgb8))
    return fail(RT_HIP_EINVAL, "an output image needs its tile buffer");
  if (tile_count == 0 || (!d_image_rgb && !d_image_rgb8))
    return RT_HIP_OK;
  const uint64_t n_tiles = (uint64_t)tiles_x_of(width) * tiles_y_of(height);
  if ((uint64_t)tile_first + (uint64_t)(tile_count - 1) * tile_stride >= n_tiles)
    return fail(RT_HIP_EINVAL, "tile range exceeds the image");
  return launched(pt_launch_untile(d_tiles_rgb, d_tiles_rgb8, width, height, tile_first, tile_stride, tile_count,
                                  d_image_rgb, d_image_rgb8, static_cast<hipStream_t>(stream)), "pt_untile");
}

/* ---- first-hit feature buffers (rt_hip.h, RtHipAov) ----------------------------------------------------------------------
 * The launch takes launch_prepare's camera-dependent fields and acquire_tables' filter, hierarchy and fp32 triangle table -- what
 * the beauty kernels' intersect() reads -- and nothing else: not pt_plan_launch (the AOV forms are no rows of the pick table, the
 * scene alone picks one: pt_aov_pick), nor launch_device_state (the body needs neither the status word nor the parked-walk
 * workspace: it cannot fail on the device and walks the hierarchy per lane). */
const char *rt_hip_aov_kernel_name(const RtHipScene *scene) { return scene ? pt_aov_kernel_name_of(pt_aov_pick(scene->view)) : ""; }

int rt_hip_aov_kernel_count(void) { return pt_aov_kernel_count(); }

const char *rt_hip_aov_kernel_launches(int index, uint64_t *launches)
{
  return kernel_launches_of(index, launches, pt_aov_kernel_count(), pt_aov_kernel_name_of, pt_aov_kernel_launches);
}

int rt_hip_render_aov_tiles(const RtHipScene *scene, const RtHipCamera *camera, const RtHipParams *params, const RtHipAov *d_tiles,
                            void *stream)
{
  if (!scene || !camera || !params)
    return fail(RT_HIP_EINVAL, "scene, camera and params are required");
  if (!aov_any(d_tiles))
    return fail(RT_HIP_EINVAL, "d_tiles: at least one output buffer is required");
  return guarded("rt_hip_render_aov_tiles", [&]() -> int {
    RtHipParams p = *params;
    p.max_depth = 0; /* ignored: one intersect() per sample */
    p.integrator = RT_HIP_TRACE_PATH;
    PtLaunch L;
    bool empty = false;
    int rc = launch_prepare(scene, camera, &p, L, &empty);
    if (rc || empty)
      return rc;
    const PtAovOut out = {d_tiles->albedo, d_tiles->normal, d_tiles->depth, d_tiles->object, d_tiles->hits};
    const int which = pt_aov_pick(scene->view);
    return launch_with_tables(scene, L, static_cast<hipStream_t>(stream), pt_aov_kernel_name_of(which),
                              [&] { return pt_launch_aov(L, out, static_cast<hipStream_t>(stream), which); });
  });
}

void rt_hip_query_defaults(RtHipQueryParams *params)
{
  if (!params)
    return;
  params->source = RT_HIP_RAYS_GIVEN;
  params->flags = 0u;
  params->camera = nullptr;
  params->origin_radius = 0.0;
}

const char *rt_hip_query_kernel_name(const RtHipScene *scene) { return scene ? pt_query_kernel_name_of(pt_query_pick(scene->view)) : ""; }

int rt_hip_query_kernel_count(void) { return pt_query_kernel_count(); }

const char *rt_hip_query_kernel_launches(int index, uint64_t *launches)
{
  return kernel_launches_of(index, launches, pt_query_kernel_count(), pt_query_kernel_name_of, pt_query_kernel_launches);
}

int rt_hip_query_rays(const RtHipScene *scene, const double *d_rays, const double *d_t_max, uint64_t n, const RtHipQueryParams *params,
                      const RtHipHits *d_hits, void *stream)
{
  if (!scene)
    return fail(RT_HIP_EINVAL, "scene is required");
  const int rc = check_query(d_rays, true, n, params, d_hits);
  if (rc || n == 0)
    return rc;
  return guarded("rt_hip_query_rays", [&] { return query_launch(scene, d_rays, d_t_max, n, params, d_hits, static_cast<hipStream_t>(stream)); });
}

int rt_hip_query_rays_host(const RtHipSphere *spheres, size_t n_spheres, const RtHipMesh *meshes, size_t n_meshes, const double *h_rays,
                           const double *h_t_max, uint64_t n, const RtHipQueryParams *params, int device, const RtHipHits *h_hits)
{
  return guarded("rt_hip_query_rays_host", [&] {
    return query_rays_host_impl(spheres, n_spheres, meshes, n_meshes, h_rays, h_t_max, n, params, device, h_hits);
  });
}

void rt_hip_trace_defaults(RtHipTraceParams *params)
{
  if (!params)
    return;
  memset(params, 0, sizeof *params);
  params->source = RT_HIP_RAYS_GIVEN;
  params->samples = 1;
  params->max_depth = 5;
  params->integrator = RT_HIP_TRACE_PATH;
}

const char *rt_hip_trace_kernel_name(const RtHipScene *scene) { return scene ? pt_trace_kernel_name_of(pt_trace_pick(scene->view)) : ""; }

int rt_hip_trace_kernel_count(void) { return pt_trace_kernel_count(); }

const char *rt_hip_trace_kernel_launches(int index, uint64_t *launches)
{
  return kernel_launches_of(index, launches, pt_trace_kernel_count(), pt_trace_kernel_name_of, pt_trace_kernel_launches);
}

int rt_hip_trace_rays(const RtHipScene *scene, const double *d_rays, uint64_t n, const RtHipTraceParams *params,
                      const RtHipRadiance *d_out, uint64_t *d_stats, void *stream)
{
  const int rc = check_trace(d_rays, true, n, params, d_out);
  if (rc)
    return rc;
  if (!scene)
    return fail(RT_HIP_EINVAL, "scene is required");
  if (n == 0)
    return RT_HIP_OK;
  return guarded("rt_hip_trace_rays", [&] { return trace_launch(scene, d_rays, n, params, d_out, d_stats, static_cast<hipStream_t>(stream)); });
}

int rt_hip_trace_rays_host(const RtHipSphere *spheres, size_t n_spheres, const RtHipMesh *meshes, size_t n_meshes, const double *h_rays,
                           uint64_t n, const RtHipTraceParams *params, int device, const RtHipRadiance *h_out, uint64_t *h_stats)
{
  return guarded("rt_hip_trace_rays_host", [&] {
    return trace_rays_host_impl(spheres, n_spheres, meshes, n_meshes, h_rays, n, params, device, h_out, h_stats);
  });
}

void rt_hip_lens_defaults(RtHipLens *lens)
{
  if (!lens)
    return;
  memset(lens, 0, sizeof *lens);
  lens->focus_distance = 1.0;
}

int rt_hip_lens_rays(const RtHipCamera *camera, const RtHipLens *lens, int32_t width, int32_t height, uint64_t seed, uint32_t sample,
                     uint32_t pixel_first, uint32_t n, double *d_rays, void *stream)
{
  int rc = check_lens(camera, lens, width, height);
  if (rc)
    return rc;
  const uint64_t n_pixels = (uint64_t)width * (uint64_t)height;
  if (((uint64_t)sample + 1u) * n_pixels > 0x100000000ull)
    return fail(RT_HIP_EINVAL, "sample %u of %llu pixels: the stream index sample x pixels + pixel must stay below 2^32", sample,
                (unsigned long long)n_pixels);
  if ((uint64_t)pixel_first + n > n_pixels)
    return fail(RT_HIP_EINVAL, "pixels [%u, +%u) exceed the frame's %llu", pixel_first, n, (unsigned long long)n_pixels);
  if (n == 0)
    return RT_HIP_OK;
  if (!d_rays || (reinterpret_cast<uintptr_t>(d_rays) & 15u))
    return fail(RT_HIP_EINVAL, "d_rays is required and must be 16-byte aligned");
  return on_device_of(d_rays, "d_rays", [&] {
    PtLensRays A = lens_args(camera, lens, width, height, seed);
    A.pixel_first = pixel_first;
    A.n = n;
    A.index_first = (uint32_t)((uint64_t)sample * n_pixels + pixel_first);
    A.rays = d_rays;
    return launched(lens_launch_rays(A, static_cast<hipStream_t>(stream)), "k_lens_rays");
  });
}

size_t rt_hip_lens_workspace_bytes(int32_t width, int32_t height, uint32_t slice_pixels)
{
  if (!frame_size_ok(width, height, 2) || slice_pixels == 0u)
    return 0;
  return lens_workspace((uint64_t)width * (uint64_t)height, slice_pixels).total;
}

int rt_hip_lens_resolve(const double *d_sum, int32_t width, int32_t height, int32_t samples, float *d_rgb, uint8_t *d_rgb8, void *stream)
{
  if (!frame_size_ok(width, height, 2))
    return fail(RT_HIP_EINVAL, "width and height must be in [2, 2^20] with fewer than 2^32 pixels");
  if (samples < 1)
    return fail(RT_HIP_EINVAL, "samples = %d must be >= 1", samples);
  if (!d_sum || (!d_rgb && !d_rgb8))
    return fail(RT_HIP_EINVAL, "d_sum and an output are required");
  return on_device_of(d_sum, "d_sum", [&]() -> int {
    return launched(lens_launch_resolve(d_sum, (uint64_t)width * (uint64_t)height, samples, d_rgb, d_rgb8, static_cast<hipStream_t>(stream)), "k_lens_resolve");
  });
}

int rt_hip_render_lens(const RtHipScene *scene, const RtHipCamera *camera, const RtHipLens *lens, const RtHipParams *params,
                       uint32_t slice_pixels, void *d_workspace, double *d_sum, float *d_rgb, uint8_t *d_rgb8, uint64_t *d_stats, void *stream)
{
  if (const int rc = check_render_lens(camera, lens, params, slice_pixels, d_sum || d_rgb || d_rgb8))
    return rc;
  if (!scene || !d_workspace)
    return fail(RT_HIP_EINVAL, "scene and d_workspace are required");
  if (const int rc = check_slice_buffers(d_workspace, d_sum))
    return rc;
  return guarded("rt_hip_render_lens", [&] {
    return render_lens_launch(scene, camera, lens, params, slice_pixels, d_workspace, d_sum, d_rgb, d_rgb8, d_stats, static_cast<hipStream_t>(stream));
  });
}

int rt_hip_render_lens_image(const RtHipSphere *spheres, size_t n_spheres, const RtHipMesh *meshes, size_t n_meshes, const RtHipCamera *camera,
                             const RtHipLens *lens, const RtHipParams *params, int device, float *h_rgb, uint8_t *h_rgb8, uint64_t *h_stats)
{
  return guarded("rt_hip_render_lens_image", [&] {
    return render_lens_image_impl(spheres, n_spheres, meshes, n_meshes, camera, lens, params, device, h_rgb, h_rgb8, h_stats);
  });
}

void rt_hip_probe_defaults(RtHipProbeParams *params)
{
  if (!params)
    return;
  memset(params, 0, sizeof *params);
  params->mode = RT_HIP_PROBE_SPHERE;
  params->samples = 64;
  params->max_depth = 5;
}

int rt_hip_probe_rays(const double *d_positions, const double *d_normals, uint64_t n_probes, const RtHipProbeParams *params, uint64_t k_first,
                      uint64_t n, double *d_rays, void *stream)
{
  int rc = check_probe(params, n_probes, d_normals != nullptr);
  if (rc)
    return rc;
  const uint64_t total = n_probes * (uint64_t)params->samples;
  if (k_first > total || n > total - k_first)
    return fail(RT_HIP_EINVAL, "rays [%llu, +%llu) exceed the %llu of %llu probes x %d samples", (unsigned long long)k_first,
                (unsigned long long)n, (unsigned long long)total, (unsigned long long)n_probes, params->samples);
  if (n > 0xFFFFFFFFull)
    return fail(RT_HIP_EINVAL, "n = %llu: a call writes fewer than 2^32 rays", (unsigned long long)n);
  if (n == 0)
    return RT_HIP_OK;
  if (!d_positions)
    return fail(RT_HIP_EINVAL, "d_positions is required");
  if (!d_rays || (reinterpret_cast<uintptr_t>(d_rays) & 15u))
    return fail(RT_HIP_EINVAL, "d_rays is required and must be 16-byte aligned");
  return on_device_of(d_rays, "d_rays", [&] {
    PtProbeRays A = probe_args(d_positions, d_normals, params);
    A.k_first = k_first;
    A.n = (uint32_t)n;
    A.rays = d_rays;
    return launched(probe_launch_rays(A, static_cast<hipStream_t>(stream)), "k_probe_rays");
  });
}

size_t rt_hip_probe_workspace_bytes(uint64_t n_probes, uint32_t mode, uint32_t slice_rays)
{
  if ((mode != RT_HIP_PROBE_SPHERE && mode != RT_HIP_PROBE_HEMISPHERE) || slice_rays == 0u || n_probes > 0x100000000ull)
    return 0;
  return probe_workspace(n_probes, mode, slice_rays).total;
}

int rt_hip_bake_probes(const RtHipScene *scene, const double *d_positions, const double *d_normals, uint64_t n_probes,
                       const RtHipProbeParams *params, uint32_t slice_rays, void *d_workspace, double *d_sum, double *d_coeff, float *d_coeff_f,
                       uint32_t *d_status, uint64_t *d_stats, void *stream)
{
  if (const int rc = check_probe(params, n_probes, d_normals != nullptr))
    return rc;
  if (slice_rays == 0u)
    return fail(RT_HIP_EINVAL, "slice_rays must be >= 1");
  if (const int rc = check_slice_buffers(d_workspace, d_sum)) /* (before the empty bake returns and before the null checks) */
    return rc;
  if (n_probes == 0)
    return RT_HIP_OK;
  if (!scene || !d_positions || !d_workspace || !d_coeff)
    return fail(RT_HIP_EINVAL, "scene, d_positions, d_workspace and d_coeff are required");
  return guarded("rt_hip_bake_probes", [&] {
    return bake_probes_launch(scene, d_positions, d_normals, n_probes, params, slice_rays, d_workspace, d_sum, d_coeff, d_coeff_f, d_status,
                              d_stats, static_cast<hipStream_t>(stream));
  });
}

int rt_hip_probe_resolve(const double *d_sum, uint64_t n_probes, uint32_t mode, int32_t samples, double *d_coeff, float *d_coeff_f, void *stream)
{
  if (mode != RT_HIP_PROBE_SPHERE && mode != RT_HIP_PROBE_HEMISPHERE)
    return fail(RT_HIP_EINVAL, "mode %u is neither RT_HIP_PROBE_SPHERE nor RT_HIP_PROBE_HEMISPHERE", mode);
  if (samples < 1)
    return fail(RT_HIP_EINVAL, "samples = %d must be >= 1", samples);
  if (n_probes > 0x100000000ull)
    return fail(RT_HIP_EINVAL, "n_probes = %llu exceeds 2^32", (unsigned long long)n_probes);
  if (n_probes == 0)
    return RT_HIP_OK;
  if (!d_sum || !d_coeff)
    return fail(RT_HIP_EINVAL, "d_sum and d_coeff are required");
  return on_device_of(d_sum, "d_sum",
                      [&] { return probe_resolve_launch(d_sum, n_probes, mode, samples, d_coeff, d_coeff_f, static_cast<hipStream_t>(stream)); });
}

int rt_hip_probe_irradiance(const double *d_coeff, uint64_t n_probes, const uint32_t *d_index, const double *d_normals, uint64_t m,
                            double *d_irradiance, void *stream)
{
  if (n_probes > 0x100000000ull || m > 0xFFFFFFFFull)
    return fail(RT_HIP_EINVAL, "n_probes = %llu, m = %llu: at most 2^32 probes and fewer than 2^32 entries", (unsigned long long)n_probes,
                (unsigned long long)m);
  if (m == 0)
    return RT_HIP_OK;
  if ((!d_coeff && n_probes != 0) || !d_index || !d_normals || !d_irradiance)
    return fail(RT_HIP_EINVAL, "d_coeff, d_index, d_normals and d_irradiance are required");
  return on_device_of(d_irradiance, "d_irradiance", [&] {
    return launched(probe_launch_irradiance(d_coeff, n_probes, d_index, d_normals, m, d_irradiance, static_cast<hipStream_t>(stream)), "k_probe_irradiance");
  });
}

int rt_hip_bake_probes_host(const RtHipSphere *spheres, size_t n_spheres, const RtHipMesh *meshes, size_t n_meshes, const double *h_positions,
                            const double *h_normals, uint64_t n_probes, const RtHipProbeParams *params, int device, double *h_coeff,
                            float *h_coeff_f, uint32_t *h_status, uint64_t *h_stats)
{
  return guarded("rt_hip_bake_probes_host", [&] {
    return bake_probes_host_impl(spheres, n_spheres, meshes, n_meshes, h_positions, h_normals, n_probes, params, device, h_coeff, h_coeff_f,
                                 h_status, h_stats);
  });
}

void rt_hip_probe_grid_defaults(RtHipProbeGrid *grid)
{
  if (!grid)
    return;
  memset(grid, 0, sizeof *grid);
  grid->struct_size = (uint32_t)sizeof *grid;
  for (int a = 0; a < 3; a++)
  {
    grid->step[a] = 1.0;
    grid->count[a] = 1u;
    grid->miss_color[a] = (float)(10.0 / 255.0);
  }
}

int rt_hip_probe_grid_positions(const RtHipProbeGrid *grid, double *d_positions, void *stream)
{
  if (const int rc = check_grid(grid))
    return rc;
  if (!d_positions)
    return fail(RT_HIP_EINVAL, "d_positions is required");
  return on_device_of(d_positions, "d_positions", [&] {
    return launched(probe_launch_grid_positions(grid_args(grid), d_positions, static_cast<hipStream_t>(stream)), "k_probe_grid_positions");
  });
}

size_t rt_hip_probe_grid_workspace_bytes(const RtHipProbeGrid *grid, uint32_t slice_rays)
{
  if (slice_rays == 0u || check_grid(grid))
    return 0;
  const uint64_t n = grid_probes(grid);
  return grid_bake_positions_at(n, slice_rays) + stage_align(24u * n);
}

int rt_hip_bake_probe_grid(const RtHipScene *scene, const RtHipProbeGrid *grid, const RtHipProbeParams *params, uint32_t slice_rays,
                           void *d_workspace, double *d_coeff, float *d_coeff_f, uint32_t *d_status, uint64_t *d_stats, void *stream)
{
  if (const int rc = check_grid_bake(grid, params))
    return rc;
  if (slice_rays == 0u)
    return fail(RT_HIP_EINVAL, "slice_rays must be >= 1");
  if (const int rc = check_slice_buffers(d_workspace, nullptr))
    return rc;
  if (!scene || !d_workspace || !d_coeff)
    return fail(RT_HIP_EINVAL, "scene, d_workspace and d_coeff are required");
  return guarded("rt_hip_bake_probe_grid", [&] {
    return bake_probe_grid_launch(scene, grid, params, slice_rays, d_workspace, d_coeff, d_coeff_f, d_status, d_stats, static_cast<hipStream_t>(stream));
  });
}

int rt_hip_probe_shade(const RtHipProbeGrid *grid, const double *d_coeff, const double *d_points, const double *d_normals,
                       const uint32_t *d_status, const float *d_albedo, const float *d_add, uint64_t m, double *d_irradiance, float *d_color,
                       void *stream)
{
  if (const int rc = check_shade(grid, d_coeff, d_points, d_normals, m, d_irradiance, d_color))
    return rc;
  if (m == 0)
    return RT_HIP_OK;
  return on_device_of(d_points, "d_points", [&] {
    return shade_launch(grid, d_coeff, d_points, d_normals, d_status, d_albedo, d_add, m, d_irradiance, d_color, static_cast<hipStream_t>(stream));
  });
}

size_t rt_hip_probe_preview_workspace_bytes(const RtHipScene *scene, int32_t width, int32_t height)
{
  (void)scene; /* (the size does not depend on the scene today) */
  if (!frame_size_ok(width, height, 2))
    return 0;
  return PreviewWorkspace((uint64_t)width * (uint64_t)height, frame_tile_pixels(width, height)).total;
}

int rt_hip_probe_preview(const RtHipScene *scene, const RtHipCamera *camera, const RtHipProbeGrid *grid, const double *d_coeff, int32_t width,
                         int32_t height, int32_t aov_samples, uint64_t seed, void *d_workspace, float *d_rgb, uint8_t *d_rgb8, void *stream)
{
  if (const int rc = check_preview(camera, grid, width, height, aov_samples))
    return rc;
  if (!scene || !d_coeff || !d_workspace || !d_rgb)
    return fail(RT_HIP_EINVAL, "scene, d_coeff, d_workspace and d_rgb are required");
  if (reinterpret_cast<uintptr_t>(d_workspace) & 15u)
    return fail(RT_HIP_EINVAL, "d_workspace must be 16-byte aligned");
  return guarded("rt_hip_probe_preview", [&] {
    return probe_preview_launch(scene, camera, grid, d_coeff, width, height, aov_samples, seed, d_workspace, d_rgb, d_rgb8,
                                static_cast<hipStream_t>(stream));
  });
}

int rt_hip_probe_preview_scene_image(const RtHipScene *scene, const RtHipCamera *camera, const RtHipProbeGrid *grid,
                                     const RtHipProbeParams *probe_params, int32_t width, int32_t height, int32_t aov_samples, float *h_rgb,
                                     uint8_t *h_rgb8, double *h_coeff, uint64_t *h_stats)
{
  return guarded("rt_hip_probe_preview_scene_image", [&] {
    return probe_preview_scene_image_impl(scene, camera, grid, probe_params, width, height, aov_samples, h_rgb, h_rgb8, h_coeff, h_stats);
  });
}

int rt_hip_probe_preview_image(const RtHipSphere *spheres, size_t n_spheres, const RtHipMesh *meshes, size_t n_meshes, const RtHipCamera *camera,
                               const RtHipProbeGrid *grid, const RtHipProbeParams *probe_params, int32_t width, int32_t height,
                               int32_t aov_samples, int device, float *h_rgb, uint8_t *h_rgb8, double *h_coeff, uint64_t *h_stats)
{
  return guarded("rt_hip_probe_preview_image", [&] {
    return probe_preview_image_impl(spheres, n_spheres, meshes, n_meshes, camera, grid, probe_params, width, height, aov_samples, device, h_rgb,
                                    h_rgb8, h_coeff, h_stats);
  });
}

void rt_hip_probe_vis_defaults(RtHipProbeVis *vis, const RtHipProbeGrid *grid)
{
  if (!vis)
    return;
  memset(vis, 0, sizeof *vis);
  vis->struct_size = (uint32_t)sizeof *vis;
  vis->res = 8u;
  vis->sharp = 5u;
  const double sx = grid ? grid->step[0] : 1.0, sy = grid ? grid->step[1] : 1.0, sz = grid ? grid->step[2] : 1.0;
  vis->d_max = 1.5 * std::sqrt((sx * sx + sy * sy) + sz * sz);
  vis->bias = 0.125 * std::min(sx, std::min(sy, sz));
  vis->floor = 0.015625; /* 2^-6 */
}

size_t rt_hip_probe_depth_workspace_bytes(uint64_t n_probes, uint32_t res, uint32_t slice_rays)
{
  if (res < PT_VIS_RES_MIN || res > PT_VIS_RES_MAX || slice_rays == 0u || n_probes > VIS_TEXELS_MAX || n_probes * res * res > VIS_TEXELS_MAX)
    return 0;
  return DepthWorkspace(slice_rays, n_probes, res).total;
}

int rt_hip_bake_probe_depth(const RtHipScene *scene, const double *d_positions, uint64_t n_probes, const RtHipProbeVis *vis,
                            const RtHipProbeParams *probe_params, uint32_t slice_rays, void *d_workspace, double *d_moments,
                            uint32_t *d_status, void *stream)
{
  if (const int rc = check_depth_bake(vis, probe_params, n_probes, slice_rays, d_workspace))
    return rc;
  if (n_probes == 0)
    return RT_HIP_OK;
  if (!scene || !d_positions || !d_workspace || !d_moments)
    return fail(RT_HIP_EINVAL, "scene, d_positions, d_workspace and d_moments are required");
  return guarded("rt_hip_bake_probe_depth", [&] {
    return bake_probe_depth_launch(scene, d_positions, n_probes, vis, probe_params, slice_rays, d_workspace, d_moments, d_status,
                                   static_cast<hipStream_t>(stream));
  });
}

size_t rt_hip_probe_grid_depth_workspace_bytes(const RtHipProbeGrid *grid, uint32_t res, uint32_t slice_rays)
{
  if (check_grid(grid))
    return 0;
  const uint64_t n = grid_probes(grid);
  const size_t bake = rt_hip_probe_depth_workspace_bytes(n, res, slice_rays);
  return bake ? bake + stage_align(24u * n) : 0;
}

int rt_hip_bake_probe_grid_depth(const RtHipScene *scene, const RtHipProbeGrid *grid, const RtHipProbeVis *vis,
                                 const RtHipProbeParams *probe_params, uint32_t slice_rays, void *d_workspace, double *d_moments,
                                 uint32_t *d_status, void *stream)
{
  if (const int rc = check_grid_depth_bake(grid, vis, probe_params, slice_rays, d_workspace))
    return rc;
  if (!scene || !d_workspace || !d_moments)
    return fail(RT_HIP_EINVAL, "scene, d_workspace and d_moments are required");
  return guarded("rt_hip_bake_probe_grid_depth", [&] {
    return bake_probe_grid_depth_launch(scene, grid, vis, probe_params, slice_rays, d_workspace, d_moments, d_status,
                                        static_cast<hipStream_t>(stream));
  });
}

int rt_hip_probe_shade_vis(const RtHipProbeGrid *grid, const RtHipProbeVis *vis, const double *d_coeff, const double *d_moments,
                           const double *d_points, const double *d_normals, const uint32_t *d_status, const float *d_albedo,
                           const float *d_add, uint64_t m, double *d_irradiance, float *d_color, void *stream)
{
  if (const int rc = check_shade(grid, d_coeff, d_points, d_normals, m, d_irradiance, d_color))
    return rc;
  if (const int rc = check_vis(vis, grid_probes(grid)))
    return rc;
  if (!d_moments)
    return fail(RT_HIP_EINVAL, "d_moments is required");
  if (m == 0)
    return RT_HIP_OK;
  return on_device_of(d_points, "d_points", [&] {
    return shade_vis_launch(grid, vis, d_coeff, d_moments, d_points, d_normals, d_status, d_albedo, d_add, m, d_irradiance, d_color,
                            static_cast<hipStream_t>(stream));
  });
}

int rt_hip_probe_preview_vis(const RtHipScene *scene, const RtHipCamera *camera, const RtHipProbeGrid *grid, const RtHipProbeVis *vis,
                             const double *d_coeff, const double *d_moments, int32_t width, int32_t height, int32_t aov_samples,
                             uint64_t seed, void *d_workspace, float *d_rgb, uint8_t *d_rgb8, void *stream)
{
  if (const int rc = check_preview(camera, grid, width, height, aov_samples))
    return rc;
  if (const int rc = check_vis(vis, grid_probes(grid)))
    return rc;
  if (!scene || !d_coeff || !d_moments || !d_workspace || !d_rgb)
    return fail(RT_HIP_EINVAL, "scene, d_coeff, d_moments, d_workspace and d_rgb are required");
  if (reinterpret_cast<uintptr_t>(d_workspace) & 15u)
    return fail(RT_HIP_EINVAL, "d_workspace must be 16-byte aligned");
  return guarded("rt_hip_probe_preview_vis", [&] {
    return probe_preview_launch(scene, camera, grid, d_coeff, width, height, aov_samples, seed, d_workspace, d_rgb, d_rgb8,
                                static_cast<hipStream_t>(stream), vis, d_moments);
  });
}

int rt_hip_probe_preview_vis_scene_image(const RtHipScene *scene, const RtHipCamera *camera, const RtHipProbeGrid *grid,
                                         const RtHipProbeVis *vis, const RtHipProbeParams *probe_params, int32_t width, int32_t height,
                                         int32_t aov_samples, float *h_rgb, uint8_t *h_rgb8, double *h_coeff, double *h_moments,
                                         uint64_t *h_stats)
{
  return guarded("rt_hip_probe_preview_vis_scene_image", [&]() -> int {
    if (const int rc = check_preview_vis_image(camera, grid, vis, probe_params, width, height, aov_samples, h_rgb, h_rgb8))
      return rc;
    if (!scene)
      return fail(RT_HIP_EINVAL, "scene is required");
    DeviceScope scope(scene->device);
    HIP_TRY(scope.status);
    return preview_vis_image_of(scene, scene->device, camera, grid, vis, probe_params, width, height, aov_samples, h_rgb, h_rgb8, h_coeff,
                                h_moments, h_stats);
  });
}

int rt_hip_probe_preview_vis_image(const RtHipSphere *spheres, size_t n_spheres, const RtHipMesh *meshes, size_t n_meshes,
                                   const RtHipCamera *camera, const RtHipProbeGrid *grid, const RtHipProbeVis *vis,
                                   const RtHipProbeParams *probe_params, int32_t width, int32_t height, int32_t aov_samples, int device,
                                   float *h_rgb, uint8_t *h_rgb8, double *h_coeff, double *h_moments, uint64_t *h_stats)
{
  return guarded("rt_hip_probe_preview_vis_image", [&]() -> int {
    if (const int rc = check_preview_vis_image(camera, grid, vis, probe_params, width, height, aov_samples, h_rgb, h_rgb8))
      return rc;
    return with_owned_scene(spheres, n_spheres, meshes, n_meshes, device, [&](const RtHipScene *scene, int phys) {
      return preview_vis_image_of(scene, phys, camera, grid, vis, probe_params, width, height, aov_samples, h_rgb, h_rgb8, h_coeff, h_moments,
                                  h_stats);
    });
  });
}

void rt_hip_probe_update_defaults(RtHipProbeUpdate *upd)
{
  if (!upd)
    return;
  memset(upd, 0, sizeof *upd);
  upd->struct_size = (uint32_t)sizeof *upd;
  upd->stride = 1u;
  upd->hysteresis = 0.9;
}

uint64_t rt_hip_probe_update_count(const RtHipProbeGrid *grid, const RtHipProbeUpdate *upd)
{
  if (check_grid(grid) || check_update(upd))
    return 0;
  return round_args(grid, upd).m;
}

size_t rt_hip_probe_update_workspace_bytes(const RtHipProbeGrid *grid, const RtHipProbeVis *vis, const RtHipProbeUpdate *upd,
                                           uint32_t slice_rays)
{
  if (slice_rays == 0u || check_grid(grid) || check_update(upd) || (vis && check_vis(vis, grid_probes(grid))))
    return 0;
  return update_workspace(round_args(grid, upd).m, slice_rays, 0u, vis ? vis->res : 0u).total;
}

int rt_hip_probe_grid_update(const RtHipScene *scene, const RtHipProbeGrid *grid, const RtHipProbeVis *vis,
                             const RtHipProbeParams *probe_params, const RtHipProbeUpdate *upd, uint32_t slice_rays, void *d_workspace,
                             double *d_coeff, float *d_coeff_f, double *d_moments, uint32_t *d_age, double *d_change, uint32_t *d_status,
                             uint64_t *d_stats, void *stream)
{
  if (const int rc = check_grid_update(grid, vis, probe_params, upd, slice_rays, d_workspace))
    return rc;
  if ((vis != nullptr) != (d_moments != nullptr))
    return fail(RT_HIP_EINVAL, "vis and d_moments go together");
  if (!scene || !d_workspace || !d_coeff || !d_age)
    return fail(RT_HIP_EINVAL, "scene, d_workspace, d_coeff and d_age are required");
  if (reinterpret_cast<uintptr_t>(d_moments) & 15u) /* (the moment blend moves a pair as 16 bytes) */
    return fail(RT_HIP_EINVAL, "d_moments must be 16-byte aligned");
  if (round_args(grid, upd).m == 0u)
    return RT_HIP_OK;
  return guarded("rt_hip_probe_grid_update", [&] {
    return grid_update_launch(scene, grid, vis, probe_params, upd, slice_rays, d_workspace, d_coeff, d_coeff_f, d_moments, d_age, d_change,
                              d_status, d_stats, static_cast<hipStream_t>(stream));
  });
}

int rt_hip_probe_blend_coeff(const double *d_sum, int32_t samples, const RtHipProbeGrid *grid, const RtHipProbeUpdate *upd,
                             const uint32_t *d_age, double *d_coeff, float *d_coeff_f, double *d_change, void *stream)
{
  if (const int rc = check_grid(grid))
    return rc;
  if (const int rc = check_update(upd))
    return rc;
  if (samples < 1)
    return fail(RT_HIP_EINVAL, "samples = %d must be >= 1", samples);
  if (!d_age || !d_coeff)
    return fail(RT_HIP_EINVAL, "d_age and d_coeff are required");
  const PtProbeRound R = round_args(grid, upd);
  if (R.m == 0u)
    return RT_HIP_OK;
  if (!d_sum)
    return fail(RT_HIP_EINVAL, "d_sum is required");
  return on_device_of(d_age, "d_age",
                      [&] { return coeff_blend_launch(d_sum, samples, R, upd, d_age, d_coeff, d_coeff_f, d_change, static_cast<hipStream_t>(stream)); });
}

int rt_hip_probe_blend_moments(const double *d_sums, const RtHipProbeGrid *grid, const RtHipProbeVis *vis, const RtHipProbeUpdate *upd,
                               const uint32_t *d_age, double *d_moments, void *stream)
{
  if (const int rc = check_grid(grid))
    return rc;
  if (const int rc = check_update(upd))
    return rc;
  if (const int rc = check_vis(vis, grid_probes(grid)))
    return rc;
  if (!d_age || !d_moments)
    return fail(RT_HIP_EINVAL, "d_age and d_moments are required");
  if (reinterpret_cast<uintptr_t>(d_moments) & 15u)
    return fail(RT_HIP_EINVAL, "d_moments must be 16-byte aligned");
  const PtProbeRound R = round_args(grid, upd);
  if (R.m == 0u)
    return RT_HIP_OK;
  if (!d_sums)
    return fail(RT_HIP_EINVAL, "d_sums is required");
  return on_device_of(d_age, "d_age",
                      [&] { return moment_blend_launch(d_sums, vis, R, upd, d_age, d_moments, static_cast<hipStream_t>(stream)); });
}

int rt_hip_probe_age_step(const RtHipProbeGrid *grid, const RtHipProbeUpdate *upd, uint32_t *d_age, void *stream)
{
  if (const int rc = check_grid(grid))
    return rc;
  if (const int rc = check_update(upd))
    return rc;
  if (!d_age)
    return fail(RT_HIP_EINVAL, "d_age is required");
  const PtProbeRound R = round_args(grid, upd);
  if (R.m == 0u)
    return RT_HIP_OK;
  return on_device_of(d_age, "d_age", [&] {
    return launched(probe_launch_age_step(R, d_age, nullptr, nullptr, static_cast<hipStream_t>(stream)), "k_probe_age_step");
  });
}

int rt_hip_probe_grid_update_host(const RtHipSphere *spheres, size_t n_spheres, const RtHipMesh *meshes, size_t n_meshes,
                                  const RtHipProbeGrid *grid, const RtHipProbeVis *vis, const RtHipProbeParams *probe_params,
                                  const RtHipProbeUpdate *upd, int device, double *h_coeff, float *h_coeff_f, double *h_moments,
                                  uint32_t *h_age, double *h_change, uint32_t *h_status, uint64_t *h_stats)
{
  return guarded("rt_hip_probe_grid_update_host", [&] {
    return grid_update_host_impl(spheres, n_spheres, meshes, n_meshes, grid, vis, probe_params, upd, device, h_coeff, h_coeff_f, h_moments,
                                 h_age, h_change, h_status, h_stats);
  });
}

int rt_hip_probe_update_preview_scene_image(const RtHipScene *scene, const RtHipCamera *camera, const RtHipProbeGrid *grid,
                                            const RtHipProbeVis *vis, const RtHipProbeParams *probe_params, const RtHipProbeUpdate *upd,
                                            int32_t width, int32_t height, int32_t aov_samples, float *h_rgb, uint8_t *h_rgb8, double *h_coeff,
                                            double *h_moments, uint32_t *h_age, uint64_t *h_stats)
{
  return guarded("rt_hip_probe_update_preview_scene_image", [&] {
    return update_preview_scene_image_impl(scene, camera, grid, vis, probe_params, upd, width, height, aov_samples, h_rgb, h_rgb8, h_coeff,
                                           h_moments, h_age, h_stats);
  });
}

int rt_hip_untile_aov(const RtHipAov *d_tiles, int32_t width, int32_t height, uint32_t tile_first, uint32_t tile_stride,
                      uint32_t tile_count, const RtHipAov *d_image, void *stream)
{
  if (!d_tiles || !d_image || width < 1 || height < 1)
    return fail(RT_HIP_EINVAL, "tile and image buffers and the image size are required");
  if (tile_count == 0)
    return RT_HIP_OK;
  if (tile_stride == 0 && tile_count > 1)
    return fail(RT_HIP_EINVAL, "tile_stride must be >= 1");
  const uint64_t n_tiles = (uint64_t)tiles_x_of(width) * tiles_y_of(height);
  if ((uint64_t)tile_first + (uint64_t)(tile_count - 1) * tile_stride >= n_tiles)
    return fail(RT_HIP_EINVAL, "tile range exceeds the image");
  const void *src[5] = {d_tiles->albedo, d_tiles->normal, d_tiles->depth, d_tiles->object, d_tiles->hits};
  void *dst[5] = {d_image->albedo, d_image->normal, d_image->depth, d_image->object, d_image->hits};
  for (int k = 0; k < 5; k++)
  {
    if (!src[k] || !dst[k])
      continue;
    const hipError_t e = pt_launch_untile_aov(static_cast<const uint32_t *>(src[k]), k < 2 ? 3u : 1u, width, height, tile_first,
                                              tile_stride, tile_count, static_cast<uint32_t *>(dst[k]), static_cast<hipStream_t>(stream));
    if (const int rc = launched(e, "pt_untile_aov"))
      return rc;
  }
  return RT_HIP_OK;
}

int rt_hip_render_aov_image(const RtHipSphere *spheres, size_t n_spheres, const RtHipMesh *meshes, size_t n_meshes,
                            const RtHipCamera *camera, const RtHipParams *params, int device, const RtHipAov *h_image)
{
  return guarded("rt_hip_render_aov_image",
                 [&] { return render_aov_image_impl(spheres, n_spheres, meshes, n_meshes, camera, params, device, h_image); });
}

/* rt_hip_render_adaptive_image: a scene and an accumulation of their own on the logical device, the driver, the frame and the count
 * map to host arrays.  Synchronous on the null stream. */
int rt_hip_render_adaptive_image(const RtHipSphere *spheres, size_t n_spheres, const RtHipMesh *meshes, size_t n_meshes,
                                 const RtHipCamera *camera, const RtHipParams *params, const RtHipAdaptParams *adapt, int device,
                                 float *h_rgb, uint8_t *h_rgb8, uint32_t *h_tile_samples, uint64_t *h_stats, double *kernel_seconds,
                                 int (*on_checkpoint)(void *user, int32_t samples_done, uint32_t live_tiles), void *user)
{
  if (kernel_seconds)
    *kernel_seconds = 0;
  if (!camera || !params || (!h_rgb && !h_rgb8))
    return fail(RT_HIP_EINVAL, "camera, params and an output image are required");
  RtHipAdaptParams defaults;
  rt_hip_adapt_defaults(&defaults);
  if (!adapt)
    adapt = &defaults;
  int rc = check_adapt(adapt);
  if (!rc)
    rc = check_params(params);
  if (rc)
    return rc;
  return guarded("rt_hip_render_adaptive_image", [&]() -> int {
    int phys = -1;
    rc = physical_device(device, &phys);
    if (rc)
      return rc;
    RtHipParams p = *params;
    whole_image(p);
    OwnedScene own; /* (outlives the accumulation: destroyed when this scope ends) */
    RtHipAccum *acc = nullptr;
    uint64_t stats[RT_HIP_NSTATS] = {0, 0, 0, 0};
    rc = own.create(spheres, n_spheres, meshes, n_meshes, phys);
    if (!rc)
      rc = rt_hip_accum_create(own.scene, camera, &p, &acc);
    if (!rc)
      rc = rt_hip_accum_run_adaptive(acc, adapt, stats, kernel_seconds, on_checkpoint, user);
    const bool cancelled = rc == RT_HIP_ECANCELLED; /* the frame of the samples done is still a whole image */
    if (!rc || cancelled)
    {
      int rc2 = rt_hip_accum_read_image(acc, h_rgb, h_rgb8);
      if (!rc2 && h_tile_samples)
        rc2 = rt_hip_accum_tile_samples(acc, h_tile_samples);
      if (rc2)
        rc = rc2;
      else if (cancelled)
        (void)fail(RT_HIP_ECANCELLED, "adaptive render cancelled: the image holds the samples done so far");
    }
    if (h_stats)
      for (int k = 0; k < RT_HIP_NSTATS; k++)
        h_stats[k] = stats[k];
    rt_hip_accum_destroy(acc);
    return rc;
  });
}

void rt_hip_denoise_defaults(RtHipDenoiseParams *params)
{
  if (!params)
    return;
  *params = RtHipDenoiseParams{};
  params->iterations = 5;
  params->flags = RT_HIP_DENOISE_DEMODULATE;
  params->normal_power_log2 = 3;
  params->sigma_color = 0.5;
  params->sigma_depth = 1.0;
}

size_t rt_hip_denoise_workspace_bytes(int32_t width, int32_t height)
{
  return frame_size_ok(width, height, 1) ? denoise_ws_bytes((size_t)width * (size_t)height) : 0u;
}

int rt_hip_denoise(const float *d_rgb, const RtHipAov *d_aov, int32_t width, int32_t height, const RtHipDenoiseParams *params,
                   void *d_workspace, float *d_out_rgb, uint8_t *d_out_rgb8, void *stream)
{
  if (const int rc = check_denoise(d_rgb, d_aov, width, height, params, d_out_rgb, d_out_rgb8))
    return rc;
  if (!d_workspace)
    return fail(RT_HIP_EINVAL, "d_workspace is required (rt_hip_denoise_workspace_bytes)");
  return on_device_of(d_rgb, "d_rgb", [&] {
    return denoise_launch(d_rgb, d_aov, width, height, params, d_workspace, d_out_rgb, d_out_rgb8, static_cast<hipStream_t>(stream));
  });
}

int rt_hip_denoise_image(const float *h_rgb, const RtHipAov *h_aov, int32_t width, int32_t height, const RtHipDenoiseParams *params,
                         int device, float *h_out_rgb, uint8_t *h_out_rgb8)
{
  return guarded("rt_hip_denoise_image",
                 [&] { return denoise_image_impl(h_rgb, h_aov, width, height, params, device, h_out_rgb, h_out_rgb8); });
}

/* the sweep of tools/reproject_bench.py (DESIGN, "`pt_reproject`") */
void rt_hip_reproject_defaults(RtHipReprojectParams *params)
{
  if (!params)
    return;
  *params = RtHipReprojectParams{};
  params->max_history = 32.0;
  params->depth_tol = 0.05;
  params->normal_min = 0.5;
}

int rt_hip_reproject(const float *d_rgb, const RtHipAov *d_aov, const RtHipCamera *camera, const float *d_hist_rgb,
                     const float *d_hist_len, const RtHipAov *d_hist_aov, const RtHipCamera *hist_camera, int32_t width, int32_t height,
                     const RtHipReprojectParams *params, float *d_out_rgb, uint8_t *d_out_rgb8, float *d_out_len, float *d_out_motion,
                     void *stream)
{
  return rt_hip_reproject_points(d_rgb, d_aov, camera, d_hist_rgb, d_hist_len, d_hist_aov, hist_camera, width, height, params, nullptr,
                                 d_out_rgb, d_out_rgb8, d_out_len, d_out_motion, stream);
}

int rt_hip_reproject_points(const float *d_rgb, const RtHipAov *d_aov, const RtHipCamera *camera, const float *d_hist_rgb,
                            const float *d_hist_len, const RtHipAov *d_hist_aov, const RtHipCamera *hist_camera, int32_t width,
                            int32_t height, const RtHipReprojectParams *params, const double *d_prev_points, float *d_out_rgb,
                            uint8_t *d_out_rgb8, float *d_out_len, float *d_out_motion, void *stream)
{
  int rc = check_reproject(d_rgb, d_aov, camera, d_hist_rgb, d_hist_len, d_hist_aov, hist_camera, width, height, params, d_out_rgb,
                           d_out_rgb8, d_out_len, d_out_motion);
  if (!rc && d_prev_points)
    rc = check_reproject_points(d_prev_points, width, height, d_out_rgb, d_out_rgb8, d_out_len, d_out_motion);
  if (rc)
    return rc;
  return on_device_of(d_rgb, "d_rgb", [&] {
    return reproject_launch(d_rgb, d_aov, camera, d_hist_rgb, d_hist_len, d_hist_aov, hist_camera, width, height, params, d_prev_points,
                            d_out_rgb, d_out_rgb8, d_out_len, d_out_motion, static_cast<hipStream_t>(stream));
  });
}

int rt_hip_reproject_image(const float *h_rgb, const RtHipAov *h_aov, const RtHipCamera *camera, const float *h_hist_rgb,
                           const float *h_hist_len, const RtHipAov *h_hist_aov, const RtHipCamera *hist_camera, int32_t width,
                           int32_t height, const RtHipReprojectParams *params, int device, float *h_out_rgb, uint8_t *h_out_rgb8,
                           float *h_out_len, float *h_out_motion)
{
  return guarded("rt_hip_reproject_image", [&] {
    return reproject_image_impl(h_rgb, h_aov, camera, h_hist_rgb, h_hist_len, h_hist_aov, hist_camera, width, height, params, nullptr,
                                device, h_out_rgb, h_out_rgb8, h_out_len, h_out_motion);
  });
}

int rt_hip_reproject_points_image(const float *h_rgb, const RtHipAov *h_aov, const RtHipCamera *camera, const float *h_hist_rgb,
                                  const float *h_hist_len, const RtHipAov *h_hist_aov, const RtHipCamera *hist_camera, int32_t width,
                                  int32_t height, const RtHipReprojectParams *params, const double *h_prev_points, int device,
                                  float *h_out_rgb, uint8_t *h_out_rgb8, float *h_out_len, float *h_out_motion)
{
  return guarded("rt_hip_reproject_points_image", [&] {
    return reproject_image_impl(h_rgb, h_aov, camera, h_hist_rgb, h_hist_len, h_hist_aov, hist_camera, width, height, params,
                                h_prev_points, device, h_out_rgb, h_out_rgb8, h_out_len, h_out_motion);
  });
}

int rt_hip_prev_points(const RtHipHits *d_hits, uint64_t n, const double *d_positions, size_t n_triangles, double *d_points, void *stream)
{
  return prev_points_device(d_hits, n, d_positions, n_triangles, nullptr, d_points, stream);
}

int rt_hip_prev_points_host(const RtHipHits *h_hits, uint64_t n, const double *h_positions, size_t n_triangles, int device, double *h_points)
{
  return guarded("rt_hip_prev_points_host",
                 [&] { return prev_points_host_impl(h_hits, n, h_positions, n_triangles, nullptr, device, h_points); });
}

int rt_hip_prev_points_moved(const RtHipHits *d_hits, uint64_t n, const double *d_positions, size_t n_triangles, const double *d_spheres_prev,
                             const double *d_spheres_cur, size_t n_spheres, double *d_points, void *stream)
{
  const MovedSpheres spheres = moved_spheres(d_spheres_prev, d_spheres_cur, n_spheres);
  return prev_points_device(d_hits, n, d_positions, n_triangles, &spheres, d_points, stream);
}

int rt_hip_prev_points_moved_host(const RtHipHits *h_hits, uint64_t n, const double *h_positions, size_t n_triangles,
                                  const double *h_spheres_prev, const double *h_spheres_cur, size_t n_spheres, int device, double *h_points)
{
  const MovedSpheres spheres = moved_spheres(h_spheres_prev, h_spheres_cur, n_spheres);
  return guarded("rt_hip_prev_points_moved_host",
                 [&] { return prev_points_host_impl(h_hits, n, h_positions, n_triangles, &spheres, device, h_points); });
}

/* k: the denoiser's; sigma_depth: the reprojection's depth tolerance (DESIGN, "`pt_upsample`") */
void rt_hip_upsample_defaults(RtHipUpsampleParams *params)
{
  if (!params)
    return;
  *params = RtHipUpsampleParams{};
  params->flags = RT_HIP_UPSAMPLE_DEMODULATE;
  params->normal_power_log2 = 3u;
  params->sigma_depth = 0.05;
}

int rt_hip_upsample(const float *d_low_rgb, const RtHipAov *d_low_aov, int32_t low_width, int32_t low_height, const RtHipAov *d_aov,
                    int32_t width, int32_t height, const RtHipUpsampleParams *params, float *d_out_rgb, uint8_t *d_out_rgb8,
                    float *d_out_conf, void *stream)
{
  if (const int rc = check_upsample(d_low_rgb, d_low_aov, low_width, low_height, d_aov, width, height, params, d_out_rgb, d_out_rgb8, d_out_conf))
    return rc;
  return on_device_of(d_low_rgb, "d_low_rgb", [&] {
    return upsample_launch(d_low_rgb, d_low_aov, low_width, low_height, d_aov, width, height, params, d_out_rgb, d_out_rgb8, d_out_conf,
                           static_cast<hipStream_t>(stream));
  });
}

int rt_hip_upsample_image(const float *h_low_rgb, const RtHipAov *h_low_aov, int32_t low_width, int32_t low_height,
                          const RtHipAov *h_aov, int32_t width, int32_t height, const RtHipUpsampleParams *params, int device,
                          float *h_out_rgb, uint8_t *h_out_rgb8, float *h_out_conf)
{
  return guarded("rt_hip_upsample_image", [&] {
    return upsample_image_impl(h_low_rgb, h_low_aov, low_width, low_height, h_aov, width, height, params, device, h_out_rgb, h_out_rgb8,
                               h_out_conf);
  });
}

size_t rt_hip_select_workspace_bytes(int32_t width, int32_t height)
{
  return frame_size_ok(width, height, 1) ? pt_select_workspace_bytes((uint64_t)width * (uint64_t)height) : 0;
}

int rt_hip_select_pixels(const float *d_values, int32_t width, int32_t height, double lo, double hi, uint32_t flags, void *d_workspace,
                         uint32_t *d_indices, uint32_t capacity, uint32_t *d_count, void *stream)
{
  if (const int rc = check_select(d_values, width, height, lo, hi, flags, d_workspace, d_indices, capacity, d_count))
    return rc;
  return on_device_of(d_values, "d_values", [&]() -> int {
    const PtSelect A = {.values = d_values, .n = (uint64_t)width * (uint64_t)height, .lo = lo, .hi = hi,
                        .invert = (flags & RT_HIP_SELECT_INVERT) ? 1u : 0u};
    const hipError_t e = pt_launch_select(A, d_workspace, d_indices, capacity, d_count, static_cast<hipStream_t>(stream));
    if (e != hipSuccess)
      return fail(RT_HIP_ERUNTIME, "pt_select launches: %s", hipGetErrorString(e));
    return RT_HIP_OK;
  });
}

void rt_hip_pixel_defaults(RtHipPixelParams *params)
{
  if (!params)
    return;
  memset(params, 0, sizeof *params);
  params->samples = 1;
  params->max_depth = 5;
  params->integrator = RT_HIP_TRACE_PATH;
}

const char *rt_hip_pixel_kernel_name(const RtHipScene *scene) { return scene ? pt_pixel_kernel_name_of(pt_trace_pick(scene->view)) : ""; }

int rt_hip_pixel_kernel_count(void) { return pt_pixel_kernel_count(); }

const char *rt_hip_pixel_kernel_launches(int index, uint64_t *launches)
{
  return kernel_launches_of(index, launches, pt_pixel_kernel_count(), pt_pixel_kernel_name_of, pt_pixel_kernel_launches);
}

int rt_hip_trace_pixels(const RtHipScene *scene, const RtHipCamera *camera, const uint32_t *d_pixels, uint64_t n,
                        const RtHipPixelParams *params, const RtHipRadiance *d_out, uint64_t *d_stats, void *stream)
{
  const int rc = check_pixels(camera, d_pixels, n, params, d_out);
  if (rc)
    return rc;
  if (!scene)
    return fail(RT_HIP_EINVAL, "scene is required");
  if (n == 0)
    return RT_HIP_OK;
  return guarded("rt_hip_trace_pixels",
                 [&] { return pixels_launch(scene, camera, d_pixels, n, params, d_out, d_stats, static_cast<hipStream_t>(stream)); });
}

int rt_hip_trace_pixels_host(const RtHipSphere *spheres, size_t n_spheres, const RtHipMesh *meshes, size_t n_meshes,
                             const RtHipCamera *camera, const uint32_t *h_pixels, uint64_t n, const RtHipPixelParams *params, int device,
                             const RtHipRadiance *h_out, uint64_t *h_stats)
{
  return guarded("rt_hip_trace_pixels_host", [&] {
    return trace_pixels_host_impl(spheres, n_spheres, meshes, n_meshes, camera, h_pixels, n, params, device, h_out, h_stats);
  });
}

int rt_hip_blend_pixels(const uint32_t *d_pixels, const uint32_t *d_status, const double *d_radiance, uint64_t n, int32_t width,
                        int32_t height, double new_weight, double prior_scale, const float *d_prior, float *d_rgb, uint8_t *d_rgb8,
                        float *d_weight, void *stream)
{
  if (const int rc = check_blend(d_pixels, d_status, d_radiance, n, width, height, new_weight, prior_scale, d_rgb))
    return rc;
  return on_device_of(d_rgb, "d_rgb", [&]() -> int { /* (the device is looked up before an empty list returns) */
    if (n == 0)
      return RT_HIP_OK;
    const PtBlend B = {.pixels = d_pixels, .status = d_status, .radiance = d_radiance, .n = n,
                       .n_pixels = (uint32_t)((uint64_t)width * (uint64_t)height), .new_weight = new_weight, .prior_scale = prior_scale,
                       .prior = d_prior, .rgb = d_rgb, .rgb8 = d_rgb8, .weight = d_weight};
    return launched(pt_launch_blend(B, static_cast<hipStream_t>(stream)), "pt_blend_pixels");
  });
}

} // extern "C"

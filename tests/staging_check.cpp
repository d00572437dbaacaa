/* staging_check.cpp -- StagePlan (raytracer.c_amd/csrc/rt_staging.h) over the part lists of the seven host-array entry points of
 * rt_hip_shim.hip, restated here by size: at 1, 63 and 65 pixels or rays, 1 and 3 samples, and every pattern of optional parts.
 * For every plan: each wanted part is 256-byte aligned and inside the total, the parts are pairwise disjoint, a part that is not
 * wanted has no offset, and the total is the sum of the aligned sizes.  Built with -fsanitize=address,undefined and run by
 * tests/test_staging_cpu.py; exits 0 and prints the number of plans checked, or prints the first violation and exits 1. */
#include "rt_staging.h"

#include <cstdio>
#include <cstdlib>
#include <utility>

namespace
{

long g_plans = 0;

struct Case
{
  const char *form;
  StagePlan plan;
  std::vector<std::pair<size_t, bool>> declared; /* bytes, wanted: what the plan was asked for */
  explicit Case(const char *f) : form(f) {}
  void add(size_t bytes, bool wanted = true)
  {
    static char host[1]; /* any non-null source and destination: the planner never reads them */
    const int k = plan.add(bytes, host, host, wanted);
    if (k != (int)declared.size())
      die("part index", (size_t)k);
    declared.push_back({bytes, wanted});
  }
  [[noreturn]] void die(const char *what, size_t part) const
  {
    fprintf(stderr, "%s: %s (part %zu of %zu, total %zu)\n", form, what, part, declared.size(), plan.total);
    exit(1);
  }
  void check() const
  {
    size_t sum = 0;
    if (plan.parts.size() != declared.size())
      die("part count", plan.parts.size());
    for (size_t k = 0; k < declared.size(); k++)
    {
      const StagePart &p = plan.parts[k];
      if (!declared[k].second)
      {
        if (plan.offset((int)k) != STAGE_ABSENT || p.src || p.dst || p.bytes)
          die("a part that is not wanted has an offset, a copy or a size", k);
        continue;
      }
      if (p.offset == STAGE_ABSENT || p.offset % 256u || p.bytes != declared[k].first)
        die("a wanted part is absent, misaligned or of another size", k);
      if (p.offset + p.bytes > plan.total || p.offset + p.bytes < p.offset)
        die("a part ends beyond the total", k);
      for (size_t q = 0; q < k; q++)
        if (declared[q].second && plan.parts[q].offset < p.offset + p.bytes && p.offset < plan.parts[q].offset + plan.parts[q].bytes)
          die("two parts overlap", k);
      sum += (p.bytes + 255u) / 256u * 256u;
    }
    if (sum != plan.total)
      die("the total is not the sum of the aligned sizes", declared.size());
    g_plans++;
  }
};

bool bit(unsigned mask, int k) { return (mask >> k) & 1u; }

void denoise(size_t n, unsigned m) /* m: demodulate, object edges, floats out (no part of its own), bytes out */
{
  Case c("denoise_image");
  c.add(3u * stage_align(16u * n) + stage_align(8u * n)); /* the workspace (denoise_ws_bytes) */
  c.add(12u * n);                                         /* colour, in and out */
  c.add(12u * n, bit(m, 0));
  c.add(12u * n);
  c.add(4u * n);
  c.add(4u * n);
  c.add(4u * n, bit(m, 1));
  c.add(3u * n, bit(m, 3));
  c.check();
}

void reproject(size_t n, unsigned m) /* m: history, motion, bytes */
{
  Case c("reproject_image");
  for (int f = 0; f < 2; f++)
    for (size_t bytes : {12u * n, 12u * n, 4u * n, 4u * n, 4u * n, 4u * n})
      c.add(bytes, f == 0 || bit(m, 0));
  c.add(8u * n, bit(m, 1));
  c.add(3u * n, bit(m, 2));
  c.check();
}

void upsample(size_t n_low, size_t n, unsigned m) /* m: demodulate, object edges, confidence, bytes */
{
  Case c("upsample_image");
  for (size_t px : {n_low, n})
  {
    c.add(12u * px, bit(m, 0));
    c.add(12u * px);
    c.add(4u * px);
    c.add(4u * px);
    c.add(4u * px, bit(m, 1));
  }
  c.add(12u * n_low);
  c.add(12u * n);
  c.add(4u * n, bit(m, 2));
  c.add(3u * n, bit(m, 3));
  c.check();
}

void aov_image(size_t n, unsigned m) /* m: albedo, normal, depth, object, hits */
{
  const size_t tile_px = (n + 63u) / 64u * 64u;
  Case c("render_aov_image");
  for (int k = 0; k < 5; k++)
  {
    c.add((k < 2 ? 12u : 4u) * tile_px, bit(m, k));
    c.add((k < 2 ? 12u : 4u) * n, bit(m, k));
  }
  c.check();
}

void query(size_t n, bool uv, unsigned m) /* m: t_max, then the eight outputs */
{
  const size_t per_ray[8] = {4, 8, 4, 4, 24, 24, 16, 48};
  Case c("query_rays_host");
  c.add((uv ? 16u : 48u) * n);
  c.add(8u * n, bit(m, 0));
  for (int k = 0; k < 8; k++)
    c.add(per_ray[k] * n, bit(m, 1 + k));
  c.check();
}

void radiance(const char *form, size_t input_bytes, size_t n, size_t samples, unsigned m, int outputs)
{
  const size_t per_entry[6] = {4, 24, 24u * samples, 8, 8, 48};
  Case c(form);
  c.add(input_bytes);
  for (int k = 0; k < 6; k++)
    c.add(per_entry[k] * n, k < outputs && bit(m, k));
  c.add(4u * sizeof(unsigned long long)); /* the counters (RT_HIP_NSTATS words) */
  c.check();
}

} // namespace

int main()
{
  const size_t counts[3] = {1, 63, 65};
  for (size_t n : counts)
  {
    for (unsigned m = 0; m < 16u; m++)
      denoise(n, m);
    for (unsigned m = 0; m < 8u; m++)
      reproject(n, m);
    for (size_t n_low : counts)
      for (unsigned m = 0; m < 16u; m++)
        upsample(n_low, n, m);
    for (unsigned m = 1; m < 32u; m++)
      aov_image(n, m);
    for (unsigned m = 2; m < 512u; m++) /* (at least one output) */
      if (m >> 1)
      {
        query(n, false, m);
        query(n, true, m);
      }
    for (size_t samples : {(size_t)1, (size_t)3})
    {
      for (unsigned m = 1; m < 64u; m++)
      {
        radiance("trace_rays_host", 48u * n, n, samples, m, 6);
        radiance("trace_rays_host (u, v)", 16u * n, n, samples, m, 6);
      }
      for (unsigned m = 1; m < 32u; m++)
        radiance("trace_pixels_host", 4u * n, n, samples, m, 5);
    }
  }
  printf("%ld plans checked\n", g_plans);
  return 0;
}

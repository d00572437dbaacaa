/* rt_staging.h -- the layout of the ONE device allocation a host-array entry point of rt_hip_shim.hip stages its arrays in.
 * A caller declares its parts in order -- bytes, the host array to upload (or none), the host array to download into (or none),
 * whether the call wants the part at all --; every wanted part gets the next 256-byte-aligned offset, a part that is not wanted
 * gets none (STAGE_ABSENT: its device pointer is null), and `total` is the sum of the aligned sizes.  Pure C++, no HIP: the
 * arithmetic that decides where a kernel writes is checked on a CPU (tests/staging_check.cpp).  StageArena (rt_hip_shim.hip) owns
 * the allocation and does the copies.  The types are hidden: the shim exports the C-ABI of rt_hip.h and nothing of this. */
#ifndef RT_STAGING_H
#define RT_STAGING_H

#include <cstddef>
#include <vector>

constexpr size_t STAGE_ALIGN = 256;
constexpr size_t STAGE_ABSENT = ~(size_t)0;

static inline size_t stage_align(size_t bytes) { return (bytes + (STAGE_ALIGN - 1)) & ~(STAGE_ALIGN - 1); }

struct __attribute__((visibility("hidden"))) StagePart
{
  size_t bytes = 0;
  const void *src = nullptr; /* host array copied to the part before the launch */
  void *dst = nullptr;       /* host array the part is copied to after it */
  bool zero = false;         /* cleared before the launch (counters) */
  size_t offset = STAGE_ABSENT;
};

struct __attribute__((visibility("hidden"))) StagePlan
{
  std::vector<StagePart> parts;
  size_t total = 0;

  /* the next part -> its index.  Not wanted: the part is kept (indices stay in declared order) without an offset, a source or
   * a destination */
  int add(size_t bytes, const void *src = nullptr, void *dst = nullptr, bool wanted = true, bool zero = false)
  {
    StagePart p;
    if (wanted)
    {
      p.bytes = bytes;
      p.src = src;
      p.dst = dst;
      p.zero = zero;
      p.offset = total;
      total += stage_align(bytes);
    }
    parts.push_back(p);
    return (int)parts.size() - 1;
  }
  size_t offset(int part) const { return parts[(size_t)part].offset; }
};

#endif

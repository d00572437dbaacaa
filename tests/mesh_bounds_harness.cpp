// CPU check of scene_mesh_centre / scene_mesh_bounds (raytracer.c_amd/csrc/bvh_build.h), the one text of what a scene derives
// from the bounds of its triangles' corners: a stand-alone program, built by tests/test_mesh_bounds_cpu.py with
// g++ -ffp-contract=off -fsanitize=address,undefined and run as a program.
// stdin: cases of 7 doubles -- lo xyz, hi xyz, r2 -- written as the 16 hex digits of their bits.
// stdout, per case, one line of hex words: scene_mesh_centre's c xyz, then scene_mesh_bounds' c xyz, R, c_norm, tau, and "1" or
// "0": round.
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "bvh_build.h"

namespace
{
void put(double d)
{
  uint64_t u;
  memcpy(&u, &d, sizeof u);
  printf("%016" PRIx64 " ", u);
}
} // namespace

int main()
{
  size_t cases = 0;
  for (;; cases++)
  {
    double in[7];
    for (int k = 0; k < 7; k++)
    {
      uint64_t u = 0;
      if (scanf("%" SCNx64, &u) != 1)
        return k == 0 && cases ? 0 : 2;
      memcpy(&in[k], &u, sizeof u);
    }
    double c[3];
    scene_mesh_centre(in, in + 3, c);
    SceneMeshBounds b;
    scene_mesh_bounds(in, in + 3, in[6], &b);
    for (double d : c)
      put(d);
    for (double d : b.c)
      put(d);
    put(b.R);
    put(b.c_norm);
    put(b.tau);
    printf("%d\n", b.round ? 1 : 0);
  }
}

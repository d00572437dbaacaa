// CPU check of scene_materials.h (raytracer.c_amd/csrc), the one text of what a scene derives from its materials: a stand-alone
// program, built by tests/material_expected.py with g++ -ffp-contract=off -fsanitize=address,undefined and run as a program.
// stdin: material lists, each "n" followed by n objects of 6 doubles (colour, emission) written as the 16 hex digits of their
// bits and the flags as a hex word.
// stdout, per list, one line of hex words: the records (8 n), the color_raw triples (3 n), max_emission, the class bits of the
// scene, then per object its class bits, its emission part, "1" or "0" (scene_material_ok) and the flags read back from its
// record.  scene_material_bounds is run over the objects scene_material_ok accepts (a created scene holds no other); a refused
// object's record is made on its own and takes no part in the scalars.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "scene_materials.h"

namespace
{
double from_bits(uint64_t u)
{
  double d;
  memcpy(&d, &u, sizeof d);
  return d;
}
void put(double d)
{
  uint64_t u;
  memcpy(&u, &d, sizeof u);
  printf("%016" PRIx64 " ", u);
}
} // namespace

int main()
{
  size_t n = 0, lists = 0;
  while (scanf("%zu", &n) == 1)
  {
    std::vector<double> in(SCENE_MATERIAL_IN * n), mat(PT_MAT_STRIDE * n), craw(3 * n);
    std::vector<uint32_t> flags(n);
    for (size_t i = 0; i < n; i++)
    {
      for (int k = 0; k < SCENE_MATERIAL_IN; k++)
      {
        uint64_t u = 0;
        if (scanf("%" SCNx64, &u) != 1)
          return 2;
        in[SCENE_MATERIAL_IN * i + k] = from_bits(u);
      }
      if (scanf("%" SCNx32, &flags[i]) != 1)
        return 2;
    }
    /* the accepted objects, gathered: the scalars are theirs */
    std::vector<double> ok_in;
    std::vector<uint32_t> ok_flags;
    for (size_t i = 0; i < n; i++)
      if (scene_material_ok(&in[SCENE_MATERIAL_IN * i], &in[SCENE_MATERIAL_IN * i + 3]))
      {
        ok_in.insert(ok_in.end(), &in[SCENE_MATERIAL_IN * i], &in[SCENE_MATERIAL_IN * i] + SCENE_MATERIAL_IN);
        ok_flags.push_back(flags[i]);
      }
    SceneMaterialBounds b, all;
    scene_material_bounds(ok_in.data(), ok_flags.data(), ok_flags.size(), nullptr, nullptr, &b);
    scene_material_bounds(in.data(), flags.data(), n, mat.data(), craw.data(), &all); /* the records and triples of every object */
    for (double d : mat)
      put(d);
    for (double d : craw)
      put(d);
    put(b.max_emission);
    printf("%x ", b.classes);
    for (size_t i = 0; i < n; i++)
    {
      const double *c = &in[SCENE_MATERIAL_IN * i];
      printf("%x ", scene_material_class_part(flags[i]));
      put(scene_material_emission_part(c + 3));
      printf("%d %x ", scene_material_ok(c, c + 3) ? 1 : 0, scene_material_flags(&mat[PT_MAT_STRIDE * i]));
    }
    printf("\n");
    lists++;
  }
  return lists ? 0 : 1;
}

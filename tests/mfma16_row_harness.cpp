// Host harness of tests/test_mfma16_table_cpu.py: pt_mfma16_row (pt_device.h), the row of the fp16 matrix form of the phase-1
// filter, for spheres read from stdin -- "cx cy cz r near_R tol" per line, hexadecimal floats allowed -- as one line each:
//   fits  16 halves (hex)  W16  A
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include "pt_device.h"

int main()
{
  char line[512];
  while (fgets(line, sizeof line, stdin))
  {
    double v[6];
    char *p = line;
    for (int k = 0; k < 6; k++)
      v[k] = strtod(p, &p);
    const double cn = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]) * (1.0 + 1e-12); // as the shim rounds |c| up
    const double src[6] = {v[0], v[1], v[2], v[3] * v[3], cn, std::fabs(v[3])};
    uint16_t row[16];
    const int fits = pt_mfma16_row(src, v[4], v[5], row);
    const double A = (cn + v[4] + v[5]) * (1.0 + 1e-6);
    printf("%d", fits);
    for (int k = 0; k < 16; k++)
      printf(" %04x", row[k]);
    printf(" %a %a\n", pt_mfma16_widen(A, std::fabs(cn * cn - src[3])), A);
  }
  return 0;
}

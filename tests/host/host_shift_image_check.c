/* A group's slot of the pool when the NCO runs behind the decimator (rdsp_fd_shift_image, csrc/rdsp_design.c) against the
 * direct sum in long double:
 *   out[r][pos] = (1/N) sum_{k<=64} g_r[k] exp(+j theta (4k - r)) exp(-j 2 pi bin(pos) k / N),  g_r[k] = h[4k - r],
 *   theta = 2 pi dphi / 2^32, the tap's phase taken as the exact 32-bit product dphi (4k - r) mod 2^32,
 * for a designed decimator and seven increments, dphi = 0 (the plain branch spectra: also against rdsp_fd_decimator_image)
 * among them.  Prints the worst error in float ulps of the branch's peak component and the time of one call; the bound is
 * argv[1] (tests/test_nco_behind_decimator.py states it).  Host code only: nothing here touches a device. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "rdsp_host.h"

#define N 512

int main(int argc, char **argv) {
  const double bound = argc > 1 ? atof(argv[1]) : 1e30;
  static float h_nat[256], hc[256], img[2 * 4 * N], out[2 * 4 * N];
  if (rdsp_design_decimator(256, 10000.0, 96000.0, 1, h_nat, hc) != 0 || rdsp_fd_decimator_image(h_nat, N, img) != 0) {
    printf("design failed\n");
    return 1;
  }
  const int P = rdsp_plan_radix(N), nt = N / P;
  const uint32_t dphis[] = {0u, rdsp_nco_dphi(12000.0, 96000.0), rdsp_nco_dphi(-5390.0, 96000.0), 1u, 0x7FFFFFFFu, 0xFFFFFFFFu, 0xC0000001u};
  const long double two_pi = 6.283185307179586476925286766559L;
  double worst = 0.0;
  for (unsigned d = 0; d < sizeof(dphis) / sizeof(dphis[0]); d++) {
    memset(out, 0xFF, sizeof(out));
    if (rdsp_fd_shift_image(h_nat, N, dphis[d], out) != 0) {
      printf("rdsp_fd_shift_image failed\n");
      return 1;
    }
    for (int r = 0; r < 4; r++) {
      static long double re[N], im[N];
      long double peak = 0.0L;
      for (int pos = 0; pos < N; pos++) {
        const int bin = rdsp_bin_of_pos(N, pos);
        long double sr = 0.0L, si = 0.0L;
        for (int k = 0; k <= 64; k++) {
          const int t = 4 * k - r;
          if (t < 0 || t >= 256) continue;
          const uint32_t ph = dphis[d] * (uint32_t)t;
          const long double turns = (long double)ph / 4294967296.0L - (long double)((bin * k) % N) / (long double)N;
          sr += (long double)h_nat[t] * cosl(two_pi * turns);
          si += (long double)h_nat[t] * sinl(two_pi * turns);
        }
        re[pos] = sr / N;
        im[pos] = si / N;
        peak = fmaxl(peak, fmaxl(fabsl(re[pos]), fabsl(im[pos])));
      }
      int ex;
      frexpl(peak, &ex);                         /* peak = m 2^ex, 0.5 <= m < 1: a float ulp there is 2^(ex - 24) */
      const long double ulp = ldexpl(1.0L, ex - 24);
      for (int t = 0; t < nt; t++)
        for (int e = 0; e < P; e++) {
          const int pos = t * P + e;
          const size_t o = 2 * ((size_t)r * N + (size_t)e * nt + (size_t)t);
          const double err = (double)(fmaxl(fabsl((long double)out[o] - re[pos]), fabsl((long double)out[o + 1] - im[pos])) / ulp);
          if (!(err <= bound)) {
            printf("dphi %08x branch %d position %d: (%.9g, %.9g) for (%.17Lg, %.17Lg): %.3f ulp of the peak\n", dphis[d], r, pos, out[o],
                   out[o + 1], re[pos], im[pos], err);
            return 1;
          }
          if (err > worst) worst = err;
          /* no shift: the image rdsp_fd_decimator_image makes, to a last bit (two summation orders) */
          if (dphis[d] == 0u && fmax(fabs((double)out[o] - (double)img[o]), fabs((double)out[o + 1] - (double)img[o + 1])) > (double)ulp) {
            printf("dphi 0 branch %d position %d: not the plain spectrum\n", r, pos);
            return 1;
          }
        }
    }
  }
  struct timespec a, b;
  const int reps = 200;
  clock_gettime(CLOCK_MONOTONIC, &a);
  for (int i = 0; i < reps; i++) rdsp_fd_shift_image(h_nat, N, dphis[1] + (uint32_t)i, out);
  clock_gettime(CLOCK_MONOTONIC, &b);
  const double us_shift = ((double)(b.tv_sec - a.tv_sec) * 1e9 + (double)(b.tv_nsec - a.tv_nsec)) / reps / 1e3;
  clock_gettime(CLOCK_MONOTONIC, &a);
  for (int i = 0; i < reps; i++) rdsp_fd_rot_image(img, N, dphis[1] + (uint32_t)i, out);
  clock_gettime(CLOCK_MONOTONIC, &b);
  const double us_rot = ((double)(b.tv_sec - a.tv_sec) * 1e9 + (double)(b.tv_nsec - a.tv_nsec)) / reps / 1e3;
  printf("OK worst %.3f float ulps of the branch's peak; one slot: shifted %.1f us, rotated %.1f us\n", worst, us_shift, us_rot);
  return 0;
}

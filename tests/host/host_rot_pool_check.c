/* A group's slot of the rotated pool (rdsp_fd_rot_image, csrc/rdsp_design.c) against rot_r G_r formed here in double:
 *   out[r][k] = G_r[k] exp(-j 2 pi (r dphi mod 2^32) / 2^32),  G = rdsp_fd_decimator_image of a designed decimator,
 * each component within half a float ulp of the product's magnitude; branch 0, and every branch at dphi = 0, to the bit.
 * Host code only: nothing here touches a device. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "rdsp_host.h"

#define N 512

int main(void) {
  static float h_nat[256], hc[256], img[2 * 4 * N], out[2 * 4 * N];
  if (rdsp_design_decimator(256, 10000.0, 96000.0, 1, h_nat, hc) != 0 || rdsp_fd_decimator_image(h_nat, N, img) != 0) {
    printf("design failed\n");
    return 1;
  }
  const uint32_t dphis[] = {0u, rdsp_nco_dphi(12000.0, 96000.0), rdsp_nco_dphi(-5390.0, 96000.0), 1u, 0x7FFFFFFFu, 0xFFFFFFFFu, 0xC0000001u};
  double worst = 0.0;
  for (unsigned d = 0; d < sizeof(dphis) / sizeof(dphis[0]); d++) {
    memset(out, 0xFF, sizeof(out));
    rdsp_fd_rot_image(img, N, dphis[d], out);
    for (int r = 0; r < 4; r++) {
      const double turns = fmod((double)dphis[d] * (double)r, 4294967296.0) / 4294967296.0;
      const double c = cos(2.0 * M_PI * turns), s = -sin(2.0 * M_PI * turns);
      for (int k = 0; k < N; k++) {
        const size_t o = 2 * ((size_t)r * N + (size_t)k);
        if (r == 0 || dphis[d] == 0u) {
          if (memcmp(&out[o], &img[o], 2 * sizeof(float)) != 0) {
            printf("dphi %08x branch %d bin %d: not a copy\n", dphis[d], r, k);
            return 1;
          }
          continue;
        }
        const double re = (double)img[o] * c - (double)img[o + 1] * s, im = (double)img[o] * s + (double)img[o + 1] * c;
        const double mag = hypot(re, im), tol = mag * 0x1p-24 + 1e-45;
        const double e = fmax(fabs((double)out[o] - re), fabs((double)out[o + 1] - im));
        if (!(e <= tol)) {
          printf("dphi %08x branch %d bin %d: (%.9g, %.9g) for (%.17g, %.17g)\n", dphis[d], r, k, out[o], out[o + 1], re, im);
          return 1;
        }
        if (mag > 0.0 && e / mag > worst) worst = e / mag;
      }
    }
  }
  printf("OK worst %.3g of the product's magnitude\n", worst);
  return 0;
}

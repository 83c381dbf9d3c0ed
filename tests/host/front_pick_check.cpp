// rdsp_front_pick (csrc/rdsp_kernels.h) over the whole grid of tests/test_front_pick.py: one line per point,
//   error family radix lean pre q4 frame      (the record's fields are printed as zeros behind an error)
// in the order of the loops below; the first line is what rdsp_experimental_build() answers (0: there is one build).
// Host code only: nothing here touches a device.
#include <cstdio>

#include "rdsp.h"
#include "rdsp_kernels.h"

int main() {
  static const float2 some_mask[1] = {};
  const int fft_ls[] = {256, 512, 1024, 2048, 4096, 300};
  const int decims[] = {1, 4, 2};
  printf("experimental %d\n", rdsp_experimental_build());
  for (int fft_l : fft_ls)
    for (int decim : decims)
      for (int lean = 0; lean < 2; lean++)
        for (int fir_fd = 0; fir_fd <= 4; fir_fd++)
          for (int fir_matrix = 0; fir_matrix < 2; fir_matrix++)
            for (int nb_on = 0; nb_on < 2; nb_on++)
              for (int to_mid = 0; to_mid < 2; to_mid++)
                for (int have_rd_mask = 0; have_rd_mask < 2; have_rd_mask++)
                  for (int trigger = 0; trigger < 6; trigger++) {
                    RdspFrontParams p = {};
                    p.lean = lean;
                    p.fir_fd = fir_fd;
                    p.fir_matrix = fir_matrix;
                    p.nb_on = nb_on;
                    p.to_mid = to_mid;
                    p.rd_mask = have_rd_mask ? some_mask : nullptr;
                    // the settings of a call that changed nothing, then one of the other PRE triggers on its own
                    p.scale_i = p.scale_q = p.scale_i_hist = p.scale_q_hist = 0.5f;
                    if (trigger == 1) p.swap_iq = p.swap_hist = 1;      // swap_iq
                    if (trigger == 2) p.swap_hist = 1;                  // swap_hist != swap_iq
                    if (trigger == 3) p.scale_i_hist = 0.25f;           // scale_i_hist != scale_i
                    if (trigger == 4) p.scale_q_hist = 0.25f;           // scale_q_hist != scale_q
                    if (trigger == 5) p.scale_i = p.scale_i_hist = 1.f; // scale_i != scale_q
                    RdspFrontPick k = {-1, -1, -1, -1, -1, -1};
                    const int e = rdsp_front_pick(fft_l, decim, &p, &k);
                    if (e != 0) {
                      // a refusal leaves the record alone
                      if (k.family != -1 || k.radix != -1 || k.lean != -1 || k.pre != -1 || k.q4 != -1 || k.frame != -1) {
                        printf("record written behind error %d\n", e);
                        return 1;
                      }
                      k = RdspFrontPick{};
                    }
                    printf("%d %d %d %d %d %d %d\n", e, k.family, k.radix, k.lean, k.pre, k.q4, k.frame);
                  }
  return 0;
}

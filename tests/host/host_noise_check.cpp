/*
 * host_noise_check.cpp -- csrc/rdsp_noise.h, the arithmetic of rdsp_engine_t's noise squelch, as a program of its own: plain and
 * with -fsanitize=address,undefined.
 *
 *   host_noise_check IN OUT mode W tau_us open_n close_n hang_blocks fall rise n_rows n_blocks call_blocks
 *     IN: float32 [n_rows][n_blocks * 128], the demodulated rows.  Every row starts from a fresh channel's words (zeros) and runs
 *     through noise_reference in calls of call_blocks blocks (the last one shorter), the words handed from call to call; then
 *     once more in ONE call, which must give the same bits in every record and every word.  OUT: 32-bit words -- the key, the 65
 *     taps, then per row [n_blocks] noise, [n_blocks] nopen, [68] words as the last call left them.
 * Buffers are exactly sized heap allocations (a call's samples are copied into one of their own: a read past the call shows).
 * Prints "host_noise_check OK".
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "rdsp_noise.h"

using namespace rdsp_noise;

int main(int argc, char **argv) {
  if (argc != 14) { printf("usage: host_noise_check IN OUT mode W tau_us open_n close_n hang_blocks fall rise n_rows n_blocks call_blocks\n"); return 1; }
  const int W = atoi(argv[4]);
  const float tau_us = (float)atof(argv[5]);
  const NoiseSet set{atoi(argv[3]), (float)atof(argv[6]), (float)atof(argv[7]), atoi(argv[8]), (float)atof(argv[9]), (float)atof(argv[10])};
  const size_t n_rows = (size_t)atol(argv[11]), n_blocks = (size_t)atol(argv[12]), call_blocks = (size_t)atol(argv[13]);
  if (!squelch_ok(set.mode, set.open_n, set.close_n, set.hang_blocks, set.fall, set.rise) || !rdsp_fm::width_ok(W) || !rdsp_fm::tau_ok(tau_us) ||
      call_blocks < 1)
    return 2;
  const size_t n = n_blocks * BLOCK, per_row = 2 * n_blocks + NOISE_WORDS;
  std::vector<float> in(n_rows * n), g(NOISE_TAPS);
  std::vector<uint32_t> out(1 + NOISE_TAPS + n_rows * per_row);
  FILE *f = fopen(argv[1], "rb");
  if (!f || fread(in.data(), 4, in.size(), f) != in.size()) { printf("FAIL: cannot read %s\n", argv[1]); return 1; }
  fclose(f);
  noise_taps(tau_us, g.data());
  const uint32_t key = noise_key(set.mode, W, tau_us != 0.0f);
  out[0] = key;
  memcpy(&out[1], g.data(), NOISE_TAPS * 4);
  for (size_t r = 0; r < n_rows; r++) {
    std::vector<uint32_t> words(NOISE_WORDS, 0u), words_one(NOISE_WORDS, 0u);
    std::vector<float> nz(n_blocks), nz_one(n_blocks);
    std::vector<uint8_t> open(n_blocks), open_one(n_blocks);
    for (size_t b = 0; b < n_blocks; b += call_blocks) {
      const size_t nb = std::min(call_blocks, n_blocks - b);
      std::vector<float> call(in.begin() + (long)(r * n + b * BLOCK), in.begin() + (long)(r * n + (b + nb) * BLOCK));
      std::vector<float> cn(nb);
      std::vector<uint8_t> co(nb);
      noise_reference(g.data(), set, key, false, words.data(), call.data(), (int)nb, cn.data(), co.data());
      std::copy(cn.begin(), cn.end(), nz.begin() + (long)b);
      std::copy(co.begin(), co.end(), open.begin() + (long)b);
    }
    noise_reference(g.data(), set, key, false, words_one.data(), in.data() + r * n, (int)n_blocks, nz_one.data(), open_one.data());
    if (memcmp(nz.data(), nz_one.data(), n_blocks * 4) != 0 || open != open_one || words != words_one) {
      printf("FAIL: row %zu in calls of %zu blocks is not the row in one call\n", r, call_blocks);
      return 1;
    }
    uint32_t *o = out.data() + 1 + NOISE_TAPS + r * per_row;
    memcpy(o, nz.data(), n_blocks * 4);
    for (size_t b = 0; b < n_blocks; b++) o[n_blocks + b] = open[b];
    memcpy(o + 2 * n_blocks, words.data(), NOISE_WORDS * 4);
  }
  f = fopen(argv[2], "wb");
  if (!f || fwrite(out.data(), 4, out.size(), f) != out.size()) { printf("FAIL: cannot write %s\n", argv[2]); return 1; }
  fclose(f);
  printf("host_noise_check OK\n");
  return 0;
}

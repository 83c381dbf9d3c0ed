/*
 * host_tone_check.cpp -- csrc/rdsp_tone.h, the arithmetic of rdsp_engine_t's CTCSS tone squelch, as a program of its own: plain
 * and with -fsanitize=address,undefined.
 *
 *   host_tone_check IN OUT K on_amp off_amp n_rows n_blocks call_blocks tone_hz...
 *     IN: float32 [n_rows][n_blocks * 128], the demodulated rows; tone_hz: one per row (0: no tone).  Every row starts from a
 *     fresh channel's words (zeros) and runs through tone_reference in calls of call_blocks blocks (the last one shorter), the
 *     words handed from call to call; then once more in ONE call, which must give the same bits in every record and every
 *     word.  OUT: 32-bit words -- scale, on2, off2, then per row dphi, [n_blocks] a2, [n_blocks] tone, [8] words as the last
 *     call left them.
 * Buffers are exactly sized heap allocations (a call's samples are copied into one of their own: a read past the call shows).
 * Prints "host_tone_check OK".
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "rdsp_tone.h"

using namespace rdsp_tone;

static uint32_t word(float f) { uint32_t b; memcpy(&b, &f, 4); return b; }

int main(int argc, char **argv) {
  if (argc < 10) { printf("usage: host_tone_check IN OUT K on_amp off_amp n_rows n_blocks call_blocks tone_hz...\n"); return 1; }
  const ToneSet set{atoi(argv[3]), (float)atof(argv[4]), (float)atof(argv[5])};
  const size_t n_rows = (size_t)atol(argv[6]), n_blocks = (size_t)atol(argv[7]), call_blocks = (size_t)atol(argv[8]);
  if (!squelch_ok(set.K, set.on_amp, set.off_amp) || call_blocks < 1 || (size_t)argc != 9 + n_rows) return 2;
  std::vector<float> hz(n_rows);
  for (size_t r = 0; r < n_rows; r++) {
    hz[r] = (float)atof(argv[9 + r]);
    if (!tone_ok(hz[r])) return 2;
  }
  const ToneLaw law = tone_law(set);
  const size_t n = n_blocks * BLOCK, per_row = 1 + 2 * n_blocks + TONE_WORDS;
  std::vector<float> in(n_rows * n);
  std::vector<uint32_t> out(3 + n_rows * per_row);
  FILE *f = fopen(argv[1], "rb");
  if (!f || fread(in.data(), 4, in.size(), f) != in.size()) { printf("FAIL: cannot read %s\n", argv[1]); return 1; }
  fclose(f);
  std::vector<float4> tab(rdsp_tune::TUNE_N);
  rdsp_tune::tune_table(tab.data());
  out[0] = word(law.scale); out[1] = word(law.on2); out[2] = word(law.off2);
  for (size_t r = 0; r < n_rows; r++) {
    const uint32_t dphi = tone_dphi(hz[r]);
    std::vector<uint32_t> words(TONE_WORDS, 0u), words_one(TONE_WORDS, 0u);
    std::vector<float> a2(n_blocks), a2_one(n_blocks);
    std::vector<uint8_t> tone(n_blocks), tone_one(n_blocks);
    for (size_t b = 0; b < n_blocks; b += call_blocks) {
      const size_t nb = std::min(call_blocks, n_blocks - b);
      std::vector<float> call(in.begin() + (long)(r * n + b * BLOCK), in.begin() + (long)(r * n + (b + nb) * BLOCK));
      std::vector<float> ca(nb);
      std::vector<uint8_t> ct(nb);
      tone_reference(tab.data(), law, dphi, false, words.data(), call.data(), (int)nb, ca.data(), ct.data());
      std::copy(ca.begin(), ca.end(), a2.begin() + (long)b);
      std::copy(ct.begin(), ct.end(), tone.begin() + (long)b);
    }
    tone_reference(tab.data(), law, dphi, false, words_one.data(), in.data() + r * n, (int)n_blocks, a2_one.data(), tone_one.data());
    if (memcmp(a2.data(), a2_one.data(), n_blocks * 4) != 0 || tone != tone_one || words != words_one) {
      printf("FAIL: row %zu in calls of %zu blocks is not the row in one call\n", r, call_blocks);
      return 1;
    }
    uint32_t *o = out.data() + 3 + r * per_row;
    o[0] = dphi;
    memcpy(o + 1, a2.data(), n_blocks * 4);
    for (size_t b = 0; b < n_blocks; b++) o[1 + n_blocks + b] = tone[b];
    memcpy(o + 1 + 2 * n_blocks, words.data(), TONE_WORDS * 4);
  }
  f = fopen(argv[2], "wb");
  if (!f || fwrite(out.data(), 4, out.size(), f) != out.size()) { printf("FAIL: cannot write %s\n", argv[2]); return 1; }
  fclose(f);
  printf("host_tone_check OK\n");
  return 0;
}

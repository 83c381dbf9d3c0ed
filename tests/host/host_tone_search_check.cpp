/*
 * host_tone_search_check.cpp -- csrc/rdsp_tone_search.h, the arithmetic of rdsp_engine_t's CTCSS tone search, as a program of
 * its own: plain and with -fsanitize=address,undefined.
 *
 *   host_tone_search_check IN OUT K min_amp ratio n_rows n_blocks call_blocks tone_hz...
 *     IN: float32 [n_rows][n_blocks * 128], the demodulated rows; tone_hz: the bank (1 ... 64 tones).  Every row starts from a
 *     fresh channel's words (zeros) and runs through search_reference in calls of call_blocks blocks (the last one shorter), the
 *     words handed from call to call; then once more in ONE call, which must give the same bits in every record and every
 *     word.  OUT: 32-bit words -- scale, min2, ratio, n_tones, key, [64] dphi, then per row [n_blocks] best, [n_blocks] a2,
 *     [n_blocks] next, [200] words as the last call left them.
 * Buffers are exactly sized heap allocations (a call's samples are copied into one of their own: a read past the call shows).
 * Prints "host_tone_search_check OK".
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "rdsp_tone_search.h"

using namespace rdsp_tone_search;

static uint32_t word(float f) { uint32_t b; memcpy(&b, &f, 4); return b; }

int main(int argc, char **argv) {
  if (argc < 10) { printf("usage: host_tone_search_check IN OUT K min_amp ratio n_rows n_blocks call_blocks tone_hz...\n"); return 1; }
  const SearchSet set{atoi(argv[3]), (float)atof(argv[4]), (float)atof(argv[5])};
  const size_t n_rows = (size_t)atol(argv[6]), n_blocks = (size_t)atol(argv[7]), call_blocks = (size_t)atol(argv[8]);
  std::vector<float> hz;
  for (int k = 9; k < argc; k++) hz.push_back((float)atof(argv[k]));
  if (!search_ok(set.K, set.min_amp, set.ratio) || set.K == 0 || call_blocks < 1 || !bank_ok(hz.data(), (int)hz.size())) return 2;
  const SearchLaw law = search_law(set);
  const SearchBank bank = search_bank(hz.data(), (int)hz.size());
  const size_t n = n_blocks * BLOCK, per_row = 3 * n_blocks + SEARCH_WORDS, head = 5 + MAX_TONES;
  std::vector<float> in(n_rows * n);
  std::vector<uint32_t> out(head + n_rows * per_row);
  FILE *f = fopen(argv[1], "rb");
  if (!f || fread(in.data(), 4, in.size(), f) != in.size()) { printf("FAIL: cannot read %s\n", argv[1]); return 1; }
  fclose(f);
  std::vector<float4> tab(rdsp_tune::TUNE_N);
  rdsp_tune::tune_table(tab.data());
  out[0] = word(law.scale); out[1] = word(law.min2); out[2] = word(law.ratio); out[3] = bank.n_tones; out[4] = bank.key;
  memcpy(&out[5], bank.dphi, sizeof bank.dphi);
  for (size_t r = 0; r < n_rows; r++) {
    std::vector<uint32_t> words(SEARCH_WORDS, 0u), words_one(SEARCH_WORDS, 0u);
    std::vector<uint8_t> best(n_blocks), best_one(n_blocks);
    std::vector<float> a2(n_blocks), a2_one(n_blocks), next(n_blocks), next_one(n_blocks);
    for (size_t b = 0; b < n_blocks; b += call_blocks) {
      const size_t nb = std::min(call_blocks, n_blocks - b);
      std::vector<float> call(in.begin() + (long)(r * n + b * BLOCK), in.begin() + (long)(r * n + (b + nb) * BLOCK));
      std::vector<uint8_t> cb(nb);
      std::vector<float> ca(nb), cn(nb);
      search_reference(tab.data(), law, bank, false, words.data(), call.data(), (int)nb, cb.data(), ca.data(), cn.data());
      std::copy(cb.begin(), cb.end(), best.begin() + (long)b);
      std::copy(ca.begin(), ca.end(), a2.begin() + (long)b);
      std::copy(cn.begin(), cn.end(), next.begin() + (long)b);
    }
    search_reference(tab.data(), law, bank, false, words_one.data(), in.data() + r * n, (int)n_blocks, best_one.data(), a2_one.data(), next_one.data());
    if (best != best_one || memcmp(a2.data(), a2_one.data(), n_blocks * 4) != 0 || memcmp(next.data(), next_one.data(), n_blocks * 4) != 0 ||
        words != words_one) {
      printf("FAIL: row %zu in calls of %zu blocks is not the row in one call\n", r, call_blocks);
      return 1;
    }
    uint32_t *o = out.data() + head + r * per_row;
    for (size_t b = 0; b < n_blocks; b++) o[b] = best[b];
    memcpy(o + n_blocks, a2.data(), n_blocks * 4);
    memcpy(o + 2 * n_blocks, next.data(), n_blocks * 4);
    memcpy(o + 3 * n_blocks, words.data(), SEARCH_WORDS * 4);
  }
  f = fopen(argv[2], "wb");
  if (!f || fwrite(out.data(), 4, out.size(), f) != out.size()) { printf("FAIL: cannot write %s\n", argv[2]); return 1; }
  fclose(f);
  printf("host_tone_search_check OK\n");
  return 0;
}

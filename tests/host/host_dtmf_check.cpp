/*
 * host_dtmf_check.cpp -- csrc/rdsp_dtmf.h, the arithmetic of rdsp_engine_t's DTMF decoder, as a program of its own: plain and
 * with -fsanitize=address,undefined.
 *
 *   host_dtmf_check IN OUT K min_amp ratio twist share on_frames off_frames n_rows n_blocks call_blocks
 *     IN: float32 [n_rows][n_blocks * 128], the demodulated rows.  Every row starts from a fresh channel's words (zeros) and
 *     runs through dtmf_reference in calls of call_blocks blocks (the last one shorter), the words handed from call to call;
 *     then once more in ONE call, which must give the same bits in every record and every word.  OUT: 32-bit words -- scale,
 *     escale, min2, [8] dphi, then per row [n_blocks] key, [n_blocks] new, [n_blocks] lo, [n_blocks] hi, [168] words as the last
 *     call left them.
 * Buffers are exactly sized heap allocations (a call's samples are copied into one of their own: a read past the call shows).
 * Prints "host_dtmf_check OK".
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "rdsp_dtmf.h"

using namespace rdsp_dtmf;

static uint32_t word(float f) { uint32_t b; memcpy(&b, &f, 4); return b; }

int main(int argc, char **argv) {
  if (argc != 13) { printf("usage: host_dtmf_check IN OUT K min_amp ratio twist share on_frames off_frames n_rows n_blocks call_blocks\n"); return 1; }
  const DtmfSet set{atoi(argv[3]), (float)atof(argv[4]), (float)atof(argv[5]), (float)atof(argv[6]), (float)atof(argv[7]), atoi(argv[8]), atoi(argv[9])};
  const size_t n_rows = (size_t)atol(argv[10]), n_blocks = (size_t)atol(argv[11]), call_blocks = (size_t)atol(argv[12]);
  if (!dtmf_ok(set.K, set.min_amp, set.ratio, set.twist, set.share, set.on_frames, set.off_frames) || set.K == 0 || call_blocks < 1) return 2;
  const DtmfLaw law = dtmf_law(set);
  const size_t n = n_blocks * BLOCK, per_row = 4 * n_blocks + DTMF_WORDS, head = 3 + TONES;
  std::vector<float> in(n_rows * n);
  std::vector<uint32_t> out(head + n_rows * per_row);
  FILE *f = fopen(argv[1], "rb");
  if (!f || fread(in.data(), 4, in.size(), f) != in.size()) { printf("FAIL: cannot read %s\n", argv[1]); return 1; }
  fclose(f);
  std::vector<float4> tab(rdsp_tune::TUNE_N);
  rdsp_tune::tune_table(tab.data());
  out[0] = word(law.scale); out[1] = word(law.escale); out[2] = word(law.min2);
  memcpy(&out[3], law.dphi, sizeof law.dphi);
  for (size_t r = 0; r < n_rows; r++) {
    std::vector<uint32_t> words(DTMF_WORDS, 0u), words_one(DTMF_WORDS, 0u);
    std::vector<uint8_t> key(n_blocks), key_one(n_blocks), fresh(n_blocks), fresh_one(n_blocks);
    std::vector<float> lo(n_blocks), lo_one(n_blocks), hi(n_blocks), hi_one(n_blocks);
    for (size_t b = 0; b < n_blocks; b += call_blocks) {
      const size_t nb = std::min(call_blocks, n_blocks - b);
      std::vector<float> call(in.begin() + (long)(r * n + b * BLOCK), in.begin() + (long)(r * n + (b + nb) * BLOCK));
      std::vector<uint8_t> ck(nb), cf(nb);
      std::vector<float> cl(nb), chi(nb);
      dtmf_reference(tab.data(), law, false, words.data(), call.data(), (int)nb, ck.data(), cf.data(), cl.data(), chi.data());
      std::copy(ck.begin(), ck.end(), key.begin() + (long)b);
      std::copy(cf.begin(), cf.end(), fresh.begin() + (long)b);
      std::copy(cl.begin(), cl.end(), lo.begin() + (long)b);
      std::copy(chi.begin(), chi.end(), hi.begin() + (long)b);
    }
    dtmf_reference(tab.data(), law, false, words_one.data(), in.data() + r * n, (int)n_blocks, key_one.data(), fresh_one.data(), lo_one.data(),
                   hi_one.data());
    if (key != key_one || fresh != fresh_one || memcmp(lo.data(), lo_one.data(), n_blocks * 4) != 0 || memcmp(hi.data(), hi_one.data(), n_blocks * 4) != 0 ||
        words != words_one) {
      printf("FAIL: row %zu in calls of %zu blocks is not the row in one call\n", r, call_blocks);
      return 1;
    }
    uint32_t *o = out.data() + head + r * per_row;
    for (size_t b = 0; b < n_blocks; b++) { o[b] = key[b]; o[n_blocks + b] = fresh[b]; }
    memcpy(o + 2 * n_blocks, lo.data(), n_blocks * 4);
    memcpy(o + 3 * n_blocks, hi.data(), n_blocks * 4);
    memcpy(o + 4 * n_blocks, words.data(), DTMF_WORDS * 4);
  }
  f = fopen(argv[2], "wb");
  if (!f || fwrite(out.data(), 4, out.size(), f) != out.size()) { printf("FAIL: cannot write %s\n", argv[2]); return 1; }
  fclose(f);
  printf("host_dtmf_check OK\n");
  return 0;
}

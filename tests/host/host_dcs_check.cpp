/*
 * host_dcs_check.cpp -- csrc/rdsp_dcs.h, the arithmetic of rdsp_engine_t's DCS code squelch, as a program of its own: plain and
 * with -fsanitize=address,undefined.
 *
 *   host_dcs_check IN OUT K max_err on_hits off_hits n_rows n_blocks call_blocks code...
 *     IN: float32 [n_rows][n_blocks * 128], the demodulated rows; code: one per row as rdsp_engine_set_dcs_codes takes it, in
 *     decimal (0: none, 65535: any, + 32768: inverted).  Every row starts from a fresh channel's words (zeros) and runs through
 *     dcs_reference in calls of call_blocks blocks (the last one shorter), the words handed from call to call; then once more in
 *     ONE call, which must give the same bits in every record and every word.  OUT: 32-bit words -- step, then per row the
 *     channel's setting (dcs_sel), [n_blocks] dcs, [n_blocks] hits, [n_blocks] word, [232] words as the last call left them.
 * Buffers are exactly sized heap allocations (a call's samples are copied into one of their own: a read past the call shows).
 * Prints "host_dcs_check OK".
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "rdsp_dcs.h"

using namespace rdsp_dcs;

int main(int argc, char **argv) {
  if (argc < 11) { printf("usage: host_dcs_check IN OUT K max_err on_hits off_hits n_rows n_blocks call_blocks code...\n"); return 1; }
  const DcsSet set{atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), atoi(argv[6])};
  const size_t n_rows = (size_t)atol(argv[7]), n_blocks = (size_t)atol(argv[8]), call_blocks = (size_t)atol(argv[9]);
  if (!squelch_ok(set.K, set.max_err, set.on_hits, set.off_hits) || call_blocks < 1 || (size_t)argc != 10 + n_rows) return 2;
  std::vector<uint16_t> codes(n_rows);
  for (size_t r = 0; r < n_rows; r++) {
    const long c = atol(argv[10 + r]);
    if (c < 0 || c > 65535 || !code_ok((uint16_t)c)) return 2;
    codes[r] = (uint16_t)c;
  }
  const DcsLaw law = dcs_law(set);
  const size_t n = n_blocks * BLOCK, per_row = 1 + 3 * n_blocks + DCS_WORDS;
  std::vector<float> in(n_rows * n);
  std::vector<uint32_t> out(1 + n_rows * per_row);
  FILE *f = fopen(argv[1], "rb");
  if (!f || fread(in.data(), 4, in.size(), f) != in.size()) { printf("FAIL: cannot read %s\n", argv[1]); return 1; }
  fclose(f);
  out[0] = law.step;
  for (size_t r = 0; r < n_rows; r++) {
    const uint32_t sel = dcs_sel(codes[r]);
    std::vector<uint32_t> words(DCS_WORDS, 0u), words_one(DCS_WORDS, 0u), wrec(n_blocks), wrec_one(n_blocks);
    std::vector<uint8_t> dcs(n_blocks), dcs_one(n_blocks), hits(n_blocks), hits_one(n_blocks);
    for (size_t b = 0; b < n_blocks; b += call_blocks) {
      const size_t nb = std::min(call_blocks, n_blocks - b);
      std::vector<float> call(in.begin() + (long)(r * n + b * BLOCK), in.begin() + (long)(r * n + (b + nb) * BLOCK));
      std::vector<uint8_t> cd(nb), ch(nb);
      std::vector<uint32_t> cw(nb);
      dcs_reference(law, sel, false, words.data(), call.data(), (int)nb, cd.data(), ch.data(), cw.data());
      std::copy(cd.begin(), cd.end(), dcs.begin() + (long)b);
      std::copy(ch.begin(), ch.end(), hits.begin() + (long)b);
      std::copy(cw.begin(), cw.end(), wrec.begin() + (long)b);
    }
    dcs_reference(law, sel, false, words_one.data(), in.data() + r * n, (int)n_blocks, dcs_one.data(), hits_one.data(), wrec_one.data());
    if (dcs != dcs_one || hits != hits_one || wrec != wrec_one || words != words_one) {
      printf("FAIL: row %zu in calls of %zu blocks is not the row in one call\n", r, call_blocks);
      return 1;
    }
    uint32_t *o = out.data() + 1 + r * per_row;
    o[0] = sel;
    for (size_t b = 0; b < n_blocks; b++) { o[1 + b] = dcs[b]; o[1 + n_blocks + b] = hits[b]; o[1 + 2 * n_blocks + b] = wrec[b]; }
    memcpy(o + 1 + 3 * n_blocks, words.data(), DCS_WORDS * 4);
  }
  f = fopen(argv[2], "wb");
  if (!f || fwrite(out.data(), 4, out.size(), f) != out.size()) { printf("FAIL: cannot write %s\n", argv[2]); return 1; }
  fclose(f);
  printf("host_dcs_check OK\n");
  return 0;
}

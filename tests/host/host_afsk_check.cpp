/*
 * host_afsk_check.cpp -- csrc/rdsp_afsk.h, the arithmetic of rdsp_engine_t's AFSK 1200 packet decoder, as a program of its own:
 * plain and with -fsanitize=address,undefined.
 *
 *   host_afsk_check IN OUT space_gain pull min_bytes n_rows n_blocks
 *     IN: float32 [n_rows][n_blocks * 128], the demodulated rows.  Every row starts from a fresh channel's words (zeros) and
 *     runs through afsk_reference in ONE call; then again under every cut into calls of 1 to 3 blocks with a period of three
 *     calls (27 cuts: call k is len[k mod 3] blocks long, each len 1, 2 or 3 -- calls of one, of two and of three among them),
 *     the words handed from call to call, which must give the same bits in every record and every word.  Also the FCS of
 *     "123456789", 0x906E.  OUT: 32-bit words -- lscale, step, dphi_mark,
 *     dphi_space, then per row [n_blocks] sync, [n_blocks] new, [n_blocks] bad, [n_blocks] lvl, [448] words as the one call left
 *     them.
 * Buffers are exactly sized heap allocations (a call's samples are copied into one of their own: a read past the call shows).
 * Prints "host_afsk_check OK".
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "rdsp_afsk.h"

using namespace rdsp_afsk;

static uint32_t word(float f) { uint32_t b; memcpy(&b, &f, 4); return b; }

int main(int argc, char **argv) {
  if (argc != 8) { printf("usage: host_afsk_check IN OUT space_gain pull min_bytes n_rows n_blocks\n"); return 1; }
  const AfskSet set{1, (float)atof(argv[3]), atoi(argv[4]), atoi(argv[5])};
  const size_t n_rows = (size_t)atol(argv[6]), n_blocks = (size_t)atol(argv[7]);
  if (!afsk_ok(set.on, set.space_gain, set.pull, set.min_bytes)) return 2;
  const AfskLaw law = afsk_law(set);
  const size_t n = n_blocks * BLOCK, per_row = 4 * n_blocks + AFSK_WORDS, head = 4;
  std::vector<float> in(n_rows * n);
  std::vector<uint32_t> out(head + n_rows * per_row);
  FILE *f = fopen(argv[1], "rb");
  if (!f || fread(in.data(), 4, in.size(), f) != in.size()) { printf("FAIL: cannot read %s\n", argv[1]); return 1; }
  fclose(f);
  std::vector<float4> tab(rdsp_tune::TUNE_N);
  rdsp_tune::tune_table(tab.data());
  out[0] = word(law.lscale); out[1] = law.step; out[2] = law.dphi_mark; out[3] = law.dphi_space;
  const uint8_t check[9] = {'1', '2', '3', '4', '5', '6', '7', '8', '9'};
  if (afsk_fcs(check, 9) != 0x906Eu) { printf("FAIL: the FCS of 123456789\n"); return 1; }
  for (size_t r = 0; r < n_rows; r++) {
    std::vector<uint32_t> words_one(AFSK_WORDS, 0u);
    std::vector<uint8_t> sync_one(n_blocks), fresh_one(n_blocks), bad_one(n_blocks);
    std::vector<float> lvl_one(n_blocks);
    afsk_reference(tab.data(), law, false, words_one.data(), in.data() + r * n, (int)n_blocks, sync_one.data(), fresh_one.data(), bad_one.data(),
                   lvl_one.data());
    for (int cut = 0; cut < 27; cut++) {
      const int len[3] = {1 + cut % 3, 1 + cut / 3 % 3, 1 + cut / 9};
      std::vector<uint32_t> words(AFSK_WORDS, 0u);
      std::vector<uint8_t> sync(n_blocks), fresh(n_blocks), bad(n_blocks);
      std::vector<float> lvl(n_blocks);
      size_t call_no = 0;
      for (size_t b = 0; b < n_blocks; call_no++) {
        const size_t nb = std::min((size_t)len[call_no % 3], n_blocks - b);
        std::vector<float> call(in.begin() + (long)(r * n + b * BLOCK), in.begin() + (long)(r * n + (b + nb) * BLOCK));
        std::vector<uint8_t> cs(nb), cf(nb), cb(nb);
        std::vector<float> cl(nb);
        afsk_reference(tab.data(), law, false, words.data(), call.data(), (int)nb, cs.data(), cf.data(), cb.data(), cl.data());
        std::copy(cs.begin(), cs.end(), sync.begin() + (long)b);
        std::copy(cf.begin(), cf.end(), fresh.begin() + (long)b);
        std::copy(cb.begin(), cb.end(), bad.begin() + (long)b);
        std::copy(cl.begin(), cl.end(), lvl.begin() + (long)b);
        b += nb;
      }
      if (sync != sync_one || fresh != fresh_one || bad != bad_one || memcmp(lvl.data(), lvl_one.data(), n_blocks * 4) != 0 || words != words_one) {
        printf("FAIL: row %zu in calls of %d, %d, %d blocks is not the row in one call\n", r, len[0], len[1], len[2]);
        return 1;
      }
    }
    uint32_t *o = out.data() + head + r * per_row;
    for (size_t b = 0; b < n_blocks; b++) { o[b] = sync_one[b]; o[n_blocks + b] = fresh_one[b]; o[2 * n_blocks + b] = bad_one[b]; }
    memcpy(o + 3 * n_blocks, lvl_one.data(), n_blocks * 4);
    memcpy(o + 4 * n_blocks, words_one.data(), AFSK_WORDS * 4);
  }
  f = fopen(argv[2], "wb");
  if (!f || fwrite(out.data(), 4, out.size(), f) != out.size()) { printf("FAIL: cannot write %s\n", argv[2]); return 1; }
  fclose(f);
  printf("host_afsk_check OK\n");
  return 0;
}

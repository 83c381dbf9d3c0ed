/*
 * host_pocsag_check.cpp -- csrc/rdsp_pocsag.h, the arithmetic of rdsp_engine_t's POCSAG pager decoder, as a program of its own:
 * plain and with -fsanitize=address,undefined.
 *
 *   host_pocsag_check IN OUT baud invert pull sync_errs fix_addr fix_data n_rows n_blocks
 *     IN: float32 [n_rows][n_blocks * 128], the demodulated rows.  Every row starts from a fresh channel's words (zeros) and
 *     runs through pocsag_reference in ONE call; then again under every cut into calls of 1 to 3 blocks with a period of three
 *     calls (27 cuts: call k is len[k mod 3] blocks long, each len 1, 2 or 3 -- calls of one, of two and of three among them),
 *     the words handed from call to call, which must give the same bits in every record and every word.  Also: the sync and
 *     the idle word are codewords of their own upper 21 bits, and the table has 496 patterns.  OUT: 32-bit words -- lscale,
 *     step, then per row [n_blocks] sync, [n_blocks] new, [n_blocks] bad, [n_blocks] lvl, [n_blocks] dc, [456] words as the one
 *     call left them.
 * Buffers are exactly sized heap allocations (a call's samples are copied into one of their own: a read past the call shows).
 * Prints "host_pocsag_check OK".
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "rdsp_pocsag.h"

using namespace rdsp_pocsag;

static uint32_t word(float f) { uint32_t b; memcpy(&b, &f, 4); return b; }

struct Records {
  std::vector<uint8_t> sync, fresh, bad;
  std::vector<float> lvl, dc;
  explicit Records(size_t n) : sync(n), fresh(n), bad(n), lvl(n), dc(n) {}
  bool same(const Records &o) const {
    return sync == o.sync && fresh == o.fresh && bad == o.bad && memcmp(lvl.data(), o.lvl.data(), lvl.size() * 4) == 0 &&
           memcmp(dc.data(), o.dc.data(), dc.size() * 4) == 0;
  }
};

int main(int argc, char **argv) {
  if (argc != 11) { printf("usage: host_pocsag_check IN OUT baud invert pull sync_errs fix_addr fix_data n_rows n_blocks\n"); return 1; }
  const PocsagSet set{atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), atoi(argv[6]), atoi(argv[7]), atoi(argv[8])};
  const size_t n_rows = (size_t)atol(argv[9]), n_blocks = (size_t)atol(argv[10]);
  if (!pocsag_ok(set.baud, set.invert, set.pull, set.sync_errs, set.fix_addr, set.fix_data) || set.baud == 0) return 2;
  const PocsagLaw law = pocsag_law(set);
  const size_t n = n_blocks * BLOCK, per_row = 5 * n_blocks + POCSAG_WORDS, head = 2;
  std::vector<float> in(n_rows * n);
  std::vector<uint32_t> out(head + n_rows * per_row);
  FILE *f = fopen(argv[1], "rb");
  if (!f || fread(in.data(), 4, in.size(), f) != in.size()) { printf("FAIL: cannot read %s\n", argv[1]); return 1; }
  fclose(f);
  out[0] = word(law.lscale); out[1] = law.step;
  if (pocsag_codeword(POCSAG_SYNC >> 11) != POCSAG_SYNC || pocsag_codeword(POCSAG_IDLE >> 11) != POCSAG_IDLE) { printf("FAIL: the sync or idle word\n"); return 1; }
  int patterns = 0;
  for (int k = 1; k < 1024; k++) patterns += pocsag_table().e[k] != PG_NO_PATTERN;
  if (patterns != 496 || pocsag_table().e[0] != 0) { printf("FAIL: %d patterns\n", patterns); return 1; }
  for (size_t r = 0; r < n_rows; r++) {
    std::vector<uint32_t> words_one(POCSAG_WORDS, 0u);
    Records one(n_blocks);
    pocsag_reference(law, false, words_one.data(), in.data() + r * n, (int)n_blocks, one.sync.data(), one.fresh.data(), one.bad.data(), one.lvl.data(),
                     one.dc.data());
    for (int cut = 0; cut < 27; cut++) {
      const int len[3] = {1 + cut % 3, 1 + cut / 3 % 3, 1 + cut / 9};
      std::vector<uint32_t> words(POCSAG_WORDS, 0u);
      Records all(n_blocks);
      size_t call_no = 0;
      for (size_t b = 0; b < n_blocks; call_no++) {
        const size_t nb = std::min((size_t)len[call_no % 3], n_blocks - b);
        std::vector<float> call(in.begin() + (long)(r * n + b * BLOCK), in.begin() + (long)(r * n + (b + nb) * BLOCK));
        Records c(nb);
        pocsag_reference(law, false, words.data(), call.data(), (int)nb, c.sync.data(), c.fresh.data(), c.bad.data(), c.lvl.data(), c.dc.data());
        std::copy(c.sync.begin(), c.sync.end(), all.sync.begin() + (long)b);
        std::copy(c.fresh.begin(), c.fresh.end(), all.fresh.begin() + (long)b);
        std::copy(c.bad.begin(), c.bad.end(), all.bad.begin() + (long)b);
        std::copy(c.lvl.begin(), c.lvl.end(), all.lvl.begin() + (long)b);
        std::copy(c.dc.begin(), c.dc.end(), all.dc.begin() + (long)b);
        b += nb;
      }
      if (!all.same(one) || words != words_one) {
        printf("FAIL: row %zu in calls of %d, %d, %d blocks is not the row in one call\n", r, len[0], len[1], len[2]);
        return 1;
      }
    }
    uint32_t *o = out.data() + head + r * per_row;
    for (size_t b = 0; b < n_blocks; b++) { o[b] = one.sync[b]; o[n_blocks + b] = one.fresh[b]; o[2 * n_blocks + b] = one.bad[b]; }
    memcpy(o + 3 * n_blocks, one.lvl.data(), n_blocks * 4);
    memcpy(o + 4 * n_blocks, one.dc.data(), n_blocks * 4);
    memcpy(o + 5 * n_blocks, words_one.data(), POCSAG_WORDS * 4);
  }
  f = fopen(argv[2], "wb");
  if (!f || fwrite(out.data(), 4, out.size(), f) != out.size()) { printf("FAIL: cannot write %s\n", argv[2]); return 1; }
  fclose(f);
  printf("host_pocsag_check OK\n");
  return 0;
}

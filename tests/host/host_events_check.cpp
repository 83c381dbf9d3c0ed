/*
 * host_events_check.cpp -- csrc/rdsp_events.h, the definition of rdsp_engine_gather_events, as a program of its own: plain and
 * with -fsanitize=address,undefined.
 *
 *   host_events_check IN OUT n_channels n_blocks capacity_events capacity_words kinds
 *     IN: the three `new` records, uint8 [n_channels][n_blocks] each, then the three detector-word arrays, uint32
 *     [n_channels][168 / 448 / 456]; kinds: bit k set = kind k is on.  One events_reference call.  OUT: 32-bit words -- the five
 *     counts, the violations, then written_events records of four words and written_words payload words.
 *   host_events_check (no arguments): the cases below only.
 * Every buffer is an exactly sized heap allocation, so a read past a ring or a write past a capacity shows.  Before it reads its
 * arguments the program runs, on states of its own:
 *   - the clamp: c above n for every kind (n = 0, 1 and R - 1 under c = R + 1 and c = 255 x n_blocks) -- take is n, the
 *     violations are counted, lost stays c - min(c, R);
 *   - capacities 0, with NULL buffers: the counts of a sizing call, nothing written;
 *   - the largest slot lengths: AFSK len 328 and POCSAG n_cw 80 give 84 words, and a len or n_cw above them (which no decoder
 *     writes) still reads 84 words and no more.
 * Prints "host_events_check OK".
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "rdsp_events.h"

using namespace rdsp_events;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "host_events_check: line %d: %s\n", __LINE__, #c); exit(1); } } while (0)

struct Case {
  int n_channels, n_blocks;
  std::vector<uint8_t> fresh[KINDS];
  std::vector<uint32_t> state[KINDS];
  Case(int n, int nb) : n_channels(n), n_blocks(nb) {
    for (int k = 0; k < KINDS; k++) {
      fresh[k].assign((size_t)n * nb, k == EV_DTMF ? 255 : 0);
      state[k].assign((size_t)n * layout(k).words, 0);
    }
  }
  uint32_t *words(int k, int ch) { return state[k].data() + (size_t)ch * layout(k).words; }
  uint32_t *slot(int k, int ch, uint32_t seq) { return words(k, ch) + layout(k).ring + (size_t)(seq % layout(k).slots) * layout(k).slot_words; }
};
struct Out {
  std::vector<Record> records;
  std::vector<uint32_t> words;
  int32_t counts[5];
  int violations;
};
static Out run(const Case &c, size_t ce, size_t cw, int kinds = 7) {
  Out o;
  o.records.resize(ce);
  o.words.resize(cw);
  const uint8_t *fresh[KINDS];
  const uint32_t *state[KINDS];
  for (int k = 0; k < KINDS; k++) {
    fresh[k] = kinds >> k & 1 ? c.fresh[k].data() : nullptr;
    state[k] = kinds >> k & 1 ? c.state[k].data() : nullptr;
  }
  o.violations = events_reference(fresh, (size_t)c.n_blocks, state, c.n_channels, c.n_blocks, ce ? o.records.data() : nullptr, ce, cw ? o.words.data() : nullptr,
                                  cw, o.counts);
  return o;
}

static void clamp_cases() {
  for (int kind = 0; kind < KINDS; kind++) {
    const uint32_t R = (uint32_t)layout(kind).slots;
    const uint32_t ns[3] = {0u, 1u, R - 1u};
    for (uint32_t n : ns) {
      for (int full = 0; full < 2; full++) {
        const int nb = full ? 3 : (int)R + 1;
        Case c(2, nb);
        for (int b = 0; b < nb; b++) c.fresh[kind][(size_t)nb + b] = kind == EV_DTMF ? 5 : (full ? 255 : 1); /* channel 1 */
        const uint32_t cc = kind == EV_DTMF ? (uint32_t)nb : (full ? 255u * 3u : R + 1u);
        c.words(kind, 1)[layout(kind).count] = n;
        for (uint32_t s = 0; s < R; s++) c.slot(kind, 1, s)[0] = kind == EV_DTMF ? (7u | s << 8) : 3u;
        const Out o = run(c, 64, 64 * SLOT_MAX);
        CHECK(o.violations == (cc > n ? 1 : 0));
        const uint32_t most = cc < R ? cc : R, take = most < n ? most : n;
        CHECK(o.counts[0] == (int32_t)take && o.counts[1] == (int32_t)take);
        CHECK(o.counts[4] == (int32_t)(cc - most));
        for (uint32_t k = 0; k < take; k++)
          CHECK(o.records[k].channel == 1 && o.records[k].seq == n - take + k && (o.records[k].kind_words & 0xFFu) == (uint32_t)kind);
      }
    }
  }
}
static void sizing_case() {
  Case c(3, 5);
  c.fresh[EV_DTMF][0] = 1; c.words(EV_DTMF, 0)[layout(EV_DTMF).count] = 1; c.slot(EV_DTMF, 0, 0)[0] = 1u | 9u << 8;
  c.fresh[EV_AFSK][2 * 5 + 4] = 2; c.words(EV_AFSK, 2)[layout(EV_AFSK).count] = 7;
  c.slot(EV_AFSK, 2, 5)[0] = 17; c.slot(EV_AFSK, 2, 6)[0] = 0;
  const Out o = run(c, 0, 0);
  CHECK(o.violations == 0 && o.counts[0] == 3 && o.counts[1] == 0 && o.counts[2] == 1 + (2 + 5) + 2 && o.counts[3] == 0 && o.counts[4] == 0);
  const Out w = run(c, 3, 0); /* room for records, none for words: the first event does not fit */
  CHECK(w.counts[0] == 3 && w.counts[1] == 0 && w.counts[3] == 0);
  const Out off = run(c, 3, 10, 0); /* every kind off */
  CHECK(off.counts[0] == 0 && off.counts[2] == 0 && off.counts[4] == 0);
}
static void longest_cases() {
  const uint32_t afsk_len[3] = {328u, 329u, 0xFFFFFFFFu}, n_cw[3] = {80u, 81u, 255u};
  for (int v = 0; v < 3; v++) {
    Case c(1, 1);
    c.fresh[EV_AFSK][0] = 1; c.fresh[EV_POCSAG][0] = 1;
    c.words(EV_AFSK, 0)[layout(EV_AFSK).count] = 4; /* the ring's last slot: the state's last words */
    c.words(EV_POCSAG, 0)[layout(EV_POCSAG).count] = 4;
    uint32_t *a = c.slot(EV_AFSK, 0, 3), *p = c.slot(EV_POCSAG, 0, 3);
    for (int k = 0; k < SLOT_MAX; k++) { a[k] = 0xA0000000u + k; p[k] = 0xB0000000u + k; }
    a[0] = afsk_len[v]; p[0] = n_cw[v] | 0x10300u;
    const Out o = run(c, 2, 2 * SLOT_MAX);
    CHECK(o.violations == 0 && o.counts[0] == 2 && o.counts[1] == 2 && o.counts[2] == 2 * SLOT_MAX && o.counts[3] == 2 * SLOT_MAX);
    CHECK(o.records[0].kind_words == ((uint32_t)EV_AFSK | (uint32_t)SLOT_MAX << 8) && o.records[1].kind_words == ((uint32_t)EV_POCSAG | (uint32_t)SLOT_MAX << 8));
    CHECK(o.records[1].offset == (uint32_t)SLOT_MAX && o.records[0].seq == 3 && o.records[1].seq == 3);
    CHECK(memcmp(o.words.data(), a, SLOT_MAX * 4) == 0 && memcmp(o.words.data() + SLOT_MAX, p, SLOT_MAX * 4) == 0);
    const Out cut = run(c, 2, 2 * SLOT_MAX - 1); /* one word short: the second stays out whole */
    CHECK(cut.counts[1] == 1 && cut.counts[3] == SLOT_MAX);
  }
}

int main(int argc, char **argv) {
  clamp_cases();
  sizing_case();
  longest_cases();
  if (argc == 1) { printf("host_events_check OK\n"); return 0; }
  if (argc != 8) { fprintf(stderr, "usage: host_events_check IN OUT n_channels n_blocks capacity_events capacity_words kinds\n"); return 2; }
  const int n = atoi(argv[3]), nb = atoi(argv[4]), kinds = atoi(argv[7]);
  const long ce = atol(argv[5]), cw = atol(argv[6]);
  if (n < 1 || nb < 0 || ce < 0 || cw < 0 || kinds < 0 || kinds > 7) return 2;
  Case c(n, nb);
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  bool ok = true;
  for (int k = 0; k < KINDS; k++) ok = ok && fread(c.fresh[k].data(), 1, c.fresh[k].size(), f) == c.fresh[k].size();
  for (int k = 0; k < KINDS; k++) ok = ok && fread(c.state[k].data(), 4, c.state[k].size(), f) == c.state[k].size();
  fclose(f);
  if (!ok) return 2;
  const Out o = run(c, (size_t)ce, (size_t)cw, kinds);
  f = fopen(argv[2], "wb");
  if (!f) return 2;
  const int32_t v = o.violations;
  ok = fwrite(o.counts, 4, 5, f) == 5 && fwrite(&v, 4, 1, f) == 1;
  ok = ok && fwrite(o.records.data(), sizeof(Record), (size_t)o.counts[1], f) == (size_t)o.counts[1];
  ok = ok && fwrite(o.words.data(), 4, (size_t)o.counts[3], f) == (size_t)o.counts[3];
  if (fclose(f) != 0 || !ok) return 2;
  printf("host_events_check OK\n");
  return 0;
}

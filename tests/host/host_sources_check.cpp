// The host-only logic of the engine's source front end, from csrc/rdsp_tune.h: the workgroup run lists of the two filter-bank
// passes (source_runs) and the size of a source's history (rate_keep pairs of src_hist_words words).  A program of its own:
//   hipcc -O2 -std=c++17 --offload-arch=gfx950 -ffp-contract=off -I radiodsp_sdr_rx_amd/csrc tests/host/host_sources_check.cpp
// and the same with -Xarch_host -fsanitize=address,undefined; the vectors are sized exactly, so a run that writes past n fails there.
// Prints "host_sources_check OK" and exits 0, or the failures and 1.
#include <algorithm>
#include <cstdio>
#include <vector>

#include "rdsp_tune.h"

using namespace rdsp_tune;

static int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { printf("FAIL " __VA_ARGS__); printf("\n"); fails++; } } while (0)

// the runs of `source_of` (receivers in the engine's order: a stable sort by source) at `max` receivers a workgroup
static void check_runs(const char *name, const std::vector<int> &source_of, int max) {
  const int n = (int)source_of.size();
  std::vector<int> order((size_t)n), first((size_t)n), count((size_t)n);
  for (int c = 0; c < n; c++) order[(size_t)c] = c;
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return source_of[(size_t)a] < source_of[(size_t)b]; });
  const int runs = source_runs(order.data(), source_of.data(), n, max, first.data(), count.data());
  CHECK(runs >= 1 && runs <= n, "%s max %d: %d runs of %d receivers", name, max, runs, n);
  int at = 0;
  for (int w = 0; w < runs && w < n; w++) {
    const int f = first[(size_t)w], k = count[(size_t)w];
    CHECK(f == at, "%s max %d: run %d starts at %d, not %d (no partition in order)", name, max, w, f, at);
    CHECK(k >= 1 && k <= max && f + k <= n, "%s max %d: run %d holds %d receivers", name, max, w, k);
    if (f != at || k < 1 || f + k > n) return;
    const int src = source_of[(size_t)order[(size_t)f]];
    for (int i = f; i < f + k; i++) CHECK(source_of[(size_t)order[(size_t)i]] == src, "%s max %d: run %d mixes sources", name, max, w);
    if (w > 0) {
      const int pf = first[(size_t)w - 1], pk = count[(size_t)w - 1];
      CHECK(source_of[(size_t)order[(size_t)pf]] != src || pk == max, "%s max %d: runs %d and %d share source %d and the first holds %d", name, max,
            w - 1, w, src, pk);
    }
    at = f + k;
  }
  CHECK(at == n, "%s max %d: the runs end at %d of %d", name, max, at, n);
}

int main() {
  for (int max : {DDC_RPW, RATE_RPW}) {
    CHECK(max == (max == DDC_RPW ? 16 : 256), "the workgroup shapes moved: %d", max);
    for (int n : {max - 1, max, max + 1, 2 * max + 1}) check_runs("one source", std::vector<int>((size_t)n, 0), max);
    std::vector<int> inter((size_t)(3 * max + 5)), gap((size_t)(2 * max + 3));
    for (size_t c = 0; c < inter.size(); c++) inter[c] = (int)(c % 3);
    for (size_t c = 0; c < gap.size(); c++) gap[c] = c % 2 ? 3 : 0; // sources 1 and 2 have no receiver
    check_runs("c % 3", inter, max);
    check_runs("a source without receivers", gap, max);
    check_runs("n = 1", std::vector<int>(1, 2), max);
  }
  // one source of max + 1: exactly a full run and a run of one
  {
    int order[17], first[17], count[17];
    const std::vector<int> zero(17, 0);
    for (int c = 0; c < 17; c++) order[c] = c;
    const int runs = source_runs(order, zero.data(), 17, DDC_RPW, first, count);
    CHECK(runs == 2 && first[0] == 0 && count[0] == 16 && first[1] == 16 && count[1] == 1, "17 receivers of one source: %d runs", runs);
  }
  // the history: pairs by rate, words by format
  const struct { int P, Q, pairs; } rates[] = {{1, 1, 0}, {2, 1, 30}, {64, 1, 960}, {3, 2, 32}, {160, 147, 32}, {20480, 441, 752}};
  for (const auto &r : rates) {
    const int want = r.Q > 1 ? 16 * ((r.P + r.Q - 1) / r.Q) : r.P > 1 ? 15 * r.P : 0;
    CHECK(want == r.pairs && rate_keep(r.P, r.Q) == want, "rate_keep(%d, %d) = %d, not %d", r.P, r.Q, rate_keep(r.P, r.Q), want);
    for (int f = 0; f < SRC_FORMATS; f++) {
      const int words = rate_keep(r.P, r.Q) * src_hist_words(f);
      CHECK(words == want * (f == SRC_S16 ? 1 : 2), "history of %d / %d in format %d: %d words a source", r.P, r.Q, f, words);
    }
  }
  if (fails) return 1;
  printf("host_sources_check OK\n");
  return 0;
}

// Host restatement of rdsp_engine_t's polyphase pass for sources at 44 100 P / Q Hz (csrc/rdsp_tune.h, compiled here with
// -ffp-contract=off as the kernel is): the schedule, the prototype's taps, the chain of fmaf, the rotation and requantization.
//   host_rate_check            the checks below; prints OK
//   host_rate_check rows DIR   reads DIR/params.bin (uint32: P, Q, frac, n_out, n_rx, then n_rx x {dphi, phase}), DIR/gain.bin
//                              (one float32), DIR/src.bin (uint32 words: Tb pairs of history, then rate_pairs pairs), DIR/to.bin
//                              (float32) and DIR/station.bin (float64); writes DIR/out.bin ([n_rx][n_out] words: rate_output
//                              of every receiver), DIR/taps.bin (rate_taps(P, Q, gain)), DIR/sched.bin ([n_out] {n, r}) and
//                              DIR/dphi.bin (rate_dphi of each offset / station pair)
//   host_rate_check sched DIR  reads DIR/params.bin (uint32: P, Q, frac, n_out); writes DIR/sched.bin ([n_out] {n, r}) and
//                              DIR/pairs.bin (uint64: rate_pairs, rate_frac_after)
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "rdsp_tune.h"
using namespace rdsp_tune;

static std::vector<char> slurp(const std::string &path) {
  std::vector<char> b;
  FILE *f = fopen(path.c_str(), "rb");
  if (!f) { fprintf(stderr, "cannot read %s\n", path.c_str()); exit(2); }
  char buf[65536];
  size_t n;
  while ((n = fread(buf, 1, sizeof buf, f)) > 0) b.insert(b.end(), buf, buf + n);
  fclose(f);
  return b;
}
static void spill(const std::string &path, const void *p, size_t bytes) {
  FILE *f = fopen(path.c_str(), "wb");
  if (!f || fwrite(p, 1, bytes, f) != bytes) { fprintf(stderr, "cannot write %s\n", path.c_str()); exit(2); }
  fclose(f);
}

static int rows(const std::string &d, const float4 *tab) {
  std::vector<char> pb = slurp(d + "/params.bin"), gb = slurp(d + "/gain.bin"), sb = slurp(d + "/src.bin"), to = slurp(d + "/to.bin"),
                    st = slurp(d + "/station.bin");
  std::vector<uint32_t> par(pb.size() / 4), src(sb.size() / 4);
  memcpy(par.data(), pb.data(), par.size() * 4);
  memcpy(src.data(), sb.data(), src.size() * 4);
  float gain;
  if (par.size() < 5 || gb.size() != 4) { fprintf(stderr, "sizes\n"); return 2; }
  memcpy(&gain, gb.data(), 4);
  int P = (int)par[0], Q = (int)par[1];
  const uint32_t frac = par[2];
  const size_t n_out = par[3], n_rx = par[4], m_st = to.size() / 4;
  if (!rate_reduce(P, Q) || P != (int)par[0] || frac >= (uint32_t)Q) { fprintf(stderr, "rate\n"); return 2; }
  const int Tb = rate_tb(P, Q), Dc = rate_dc(P, Q);
  const size_t pairs = (size_t)rate_pairs(frac, P, Q, (uint32_t)n_out);
  if (par.size() != 5 + 2 * n_rx || src.size() != (size_t)Tb + pairs || st.size() != 8 * m_st) { fprintf(stderr, "sizes\n"); return 2; }
  std::vector<float> h((size_t)Tb * Q), hb((size_t)Tb);
  rate_taps(P, Q, (double)gain, h.data());
  std::vector<uint32_t> out(n_rx * n_out), dphi(m_st);
  std::vector<RateStep> sched(n_out);
  for (size_t i = 0; i < n_out; i++) {
    const RateStep s = sched[i] = rate_step(frac, P, Q, (uint32_t)i);
    if (s.n < 0 || (size_t)s.n >= pairs || s.r < 0 || s.r >= Q) { fprintf(stderr, "schedule\n"); return 2; }
    for (int j = 0; j < Tb; j++) hb[(size_t)j] = h[(size_t)j * Q + s.r];
    for (size_t r = 0; r < n_rx; r++) { /* x[0] is word Tb of src */
      const uint32_t dp = par[5 + 2 * r], ph0 = par[6 + 2 * r];
      out[r * n_out + i] = rate_output(tab, hb.data(), Tb, dp, src.data() + Tb + s.n, tune_phasor(tab, rate_phase(ph0, dp, s.n, Dc)));
    }
  }
  for (size_t k = 0; k < m_st; k++) {
    float o;
    double s;
    memcpy(&o, &to[4 * k], 4);
    memcpy(&s, &st[8 * k], 8);
    dphi[k] = rate_dphi(o, s, P, Q);
  }
  spill(d + "/out.bin", out.data(), out.size() * 4);
  spill(d + "/taps.bin", h.data(), h.size() * 4);
  spill(d + "/sched.bin", sched.data(), sched.size() * sizeof(RateStep));
  spill(d + "/dphi.bin", dphi.data(), dphi.size() * 4);
  printf("OK %d / %d, %zu receivers x %zu outputs from %zu pairs\n", P, Q, n_rx, n_out, pairs);
  return 0;
}

static int sched(const std::string &d) {
  std::vector<char> pb = slurp(d + "/params.bin");
  if (pb.size() != 16) { fprintf(stderr, "sizes\n"); return 2; }
  uint32_t par[4];
  memcpy(par, pb.data(), 16);
  const int P = (int)par[0], Q = (int)par[1];
  std::vector<RateStep> s(par[3]);
  for (uint32_t i = 0; i < par[3]; i++) s[i] = rate_step(par[2], P, Q, i);
  const uint64_t after[2] = {rate_pairs(par[2], P, Q, par[3]), rate_frac_after(par[2], P, Q, par[3])};
  spill(d + "/sched.bin", s.data(), s.size() * sizeof(RateStep));
  spill(d + "/pairs.bin", after, sizeof after);
  return 0;
}

int main(int argc, char **argv) {
  std::vector<float4> tab(TUNE_N);
  tune_table(tab.data());
  if (argc == 3 && std::string(argv[1]) == "rows") return rows(argv[2], tab.data());
  if (argc == 3 && std::string(argv[1]) == "sched") return sched(argv[2]);
  int fails = 0;

  // 1. Q = 1: the prototype is ddc_taps, the step is ddc_dphi, the schedule is the decimating pass's window
  for (int D : {1, 2, 3, 16, 64}) {
    const int T = DDC_TAPS_PER_PHASE * D;
    std::vector<float> a((size_t)T), b((size_t)T);
    ddc_taps(D, 2.5, a.data());
    rate_taps(D, 1, 2.5, b.data());
    if (memcmp(a.data(), b.data(), (size_t)T * 4) != 0) { printf("FAIL rate_taps(%d, 1) is not ddc_taps\n", D); fails++; }
    for (double s : {0.0, 200000.0, -8000.5})
      if (rate_dphi(8390.0f, s, D, 1) != ddc_dphi(8390.0f, s, D)) { printf("FAIL dphi at Q = 1\n"); fails++; }
    for (uint32_t i = 0; i < 300; i++) {
      const RateStep s = rate_step(0, D, 1, i);
      if (s.n != (int)(i + 1) * D - 1 || s.r != 0) { printf("FAIL schedule at Q = 1\n"); fails++; break; }
    }
  }
  // 2. the schedule over calls: the pairs add up to floor(M P / Q), frac stays (M P) mod Q, windows never pass the call's pairs
  for (auto pq : {std::pair<int, int>{3, 2}, {160, 147}, {20480, 441}, {441 * 64, 441}}) {
    const int P = pq.first, Q = pq.second;
    uint32_t frac = 0;
    uint64_t M = 0, total = 0;
    for (uint32_t nb : {1u, 7u, 32u, 4096u, 3u}) {
      const uint32_t n_out = nb * 128;
      const uint64_t pairs = rate_pairs(frac, P, Q, n_out);
      const RateStep last = rate_step(frac, P, Q, n_out - 1), first = rate_step(frac, P, Q, 0);
      if (first.n < 0 || (uint64_t)last.n != pairs - 1) { printf("FAIL window %d / %d\n", P, Q); fails++; }
      total += pairs; M += n_out;
      frac = rate_frac_after(frac, P, Q, n_out);
      if (total != M * (uint64_t)P / (uint64_t)Q || frac != (uint32_t)(M * (uint64_t)P % (uint64_t)Q)) { printf("FAIL pairs %d / %d\n", P, Q); fails++; }
    }
  }
  // 3. the limits
  {
    int P = 882, Q = 294;
    if (!rate_reduce(P, Q) || P != 3 || Q != 1) { printf("FAIL 882 / 294\n"); fails++; }
    const int bad[][2] = {{1, 0}, {0, 1}, {442, 442 * 2 + 1}, {885, 442}, {146, 147}, {65 * 147 + 1, 147}, {-3, 2}};
    for (auto &b : bad) {
      int p = b[0], q = b[1];
      if (rate_reduce(p, q)) { printf("FAIL %d / %d accepted\n", b[0], b[1]); fails++; }
    }
  }
  // 4. a constant source through a receiver at shift 0 comes out as the constant times the branch's sum, about the gain
  {
    const int P = 160, Q = 147, Tb = rate_tb(P, Q);
    std::vector<float> h((size_t)Tb * Q), hb((size_t)Tb);
    rate_taps(P, Q, 2.0, h.data());
    std::vector<uint32_t> x((size_t)Tb, (uint32_t)(uint16_t)(int16_t)1000 | (uint32_t)(uint16_t)(int16_t)-3000 << 16);
    for (int r : {0, 1, 73, 146}) {
      for (int j = 0; j < Tb; j++) hb[(size_t)j] = h[(size_t)j * Q + r];
      const uint32_t y = rate_output(tab.data(), hb.data(), Tb, 0u, x.data() + Tb - 1, tune_phasor(tab.data(), 0u));
      if (abs((int16_t)(uint16_t)(y & 0xffffu) - 2000) > 1 || abs((int16_t)(uint16_t)(y >> 16) + 6000) > 1) { printf("FAIL DC gain of branch %d: %08x\n", r, y); fails++; }
    }
  }
  if (fails) return 1;
  printf("OK\n");
  return 0;
}

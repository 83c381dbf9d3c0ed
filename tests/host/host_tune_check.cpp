// Host restatement of rdsp_engine_t's tuning pass (csrc/rdsp_tune.h, compiled here with -ffp-contract=off as the kernel
// is): the phasor table, the rotation and requantization, the phase accumulator.
//   host_tune_check            the checks below; prints OK
//   host_tune_check vectors D  reads D/words.bin, D/phases.bin (uint32 each), D/to.bin (float32), D/station.bin (float64);
//                              writes D/tuned.bin (tune_pair of each word at its phase), D/dphi.bin (tune_dphi of each
//                              offset / station pair) and D/table.bin (the [1024][4] float table)
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
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
static uint32_t word(int i, int q) { return (uint32_t)(uint16_t)(int16_t)i | (uint32_t)(uint16_t)(int16_t)q << 16; }
static int lo16(uint32_t w) { return (int16_t)(uint16_t)(w & 0xffffu); }
static int hi16(uint32_t w) { return (int16_t)(uint16_t)(w >> 16); }

static int vectors(const std::string &d, const float4 *tab) {
  std::vector<char> w = slurp(d + "/words.bin"), p = slurp(d + "/phases.bin"), to = slurp(d + "/to.bin"), st = slurp(d + "/station.bin");
  const size_t n = w.size() / 4, m = to.size() / 4;
  if (p.size() != w.size() || st.size() != 8 * m) { fprintf(stderr, "sizes\n"); return 2; }
  std::vector<uint32_t> out(n), dphi(m);
  for (size_t k = 0; k < n; k++) {
    uint32_t wk, pk;
    memcpy(&wk, &w[4 * k], 4);
    memcpy(&pk, &p[4 * k], 4);
    out[k] = tune_pair(wk, tune_phasor(tab, pk));
  }
  for (size_t k = 0; k < m; k++) {
    float o;
    double s;
    memcpy(&o, &to[4 * k], 4);
    memcpy(&s, &st[8 * k], 8);
    dphi[k] = tune_dphi(o, s);
  }
  spill(d + "/tuned.bin", out.data(), n * 4);
  spill(d + "/dphi.bin", dphi.data(), m * 4);
  spill(d + "/table.bin", tab, TUNE_N * sizeof(float4));
  printf("OK %zu words, %zu steps\n", n, m);
  return 0;
}

int main(int argc, char **argv) {
  std::vector<float4> tab(TUNE_N);
  tune_table(tab.data());
  if (argc == 3 && std::string(argv[1]) == "vectors") return vectors(argv[2], tab.data());
  int fails = 0;
  std::mt19937 rng(11);

  // 1. phase 0 is exactly (1, 0)
  const float2 one = tune_phasor(tab.data(), 0u);
  if (!(one.x == 1.0f && one.y == 0.0f && !std::signbit(one.y))) { printf("FAIL phase 0 gives (%a, %a)\n", one.x, one.y); fails++; }

  // 2. the phasor against cos / sin in double: every 2^9-th phase, every phase around each table entry, random phases
  double worst = 0.0;
  auto probe = [&](uint32_t ph) {
    const float2 cs = tune_phasor(tab.data(), ph);
    const double a = 2.0 * M_PI * (double)ph / 4294967296.0;
    worst = std::fmax(worst, std::fmax(std::fabs(cs.x - std::cos(a)), std::fabs(cs.y - std::sin(a))));
  };
  for (uint64_t ph = 0; ph < (1ull << 32); ph += 1u << 9) probe((uint32_t)ph);
  for (uint32_t k = 0; k < (uint32_t)TUNE_N; k++)
    for (int d = -4; d <= 4; d++) probe((k << TUNE_FRAC_BITS) + (uint32_t)d);
  for (int k = 0; k < 1000000; k++) probe((uint32_t)rng());
  printf("phasor max abs err %.3e (bound 2^-17 = %.3e)\n", worst, std::ldexp(1.0, -17));
  if (!(worst < std::ldexp(1.0, -17))) { printf("FAIL phasor error\n"); fails++; }

  // 3. shift 0 is the identity: edge pairs and random pairs
  const int edge[] = {-32768, -32767, -1, 0, 1, 32766, 32767};
  for (int i : edge)
    for (int q : edge)
      if (tune_pair(word(i, q), one) != word(i, q)) { printf("FAIL identity (%d, %d)\n", i, q); fails++; }
  for (int k = 0; k < 1000000; k++) {
    const uint32_t w = (uint32_t)rng();
    if (tune_pair(w, tune_phasor(tab.data(), 0u)) != w) { printf("FAIL identity %08x\n", w); fails++; break; }
  }

  // 4. full-scale rotations saturate (never wrap): within one count of the saturated double rotation; the corners exactly
  int sat_hits = 0, off = 0;
  const int full[] = {-32768, 32767};
  for (int i : full)
    for (int q : full)
      for (uint32_t k = 0; k < 4096; k++) {
        const uint32_t ph = k * 1048573u;
        const float2 cs = tune_phasor(tab.data(), ph);
        const uint32_t r = tune_pair(word(i, q), cs);
        const double a = 2.0 * M_PI * (double)ph / 4294967296.0;
        const double ir = i * std::cos(a) - q * std::sin(a), qr = q * std::cos(a) + i * std::sin(a);
        const double wi = std::fmin(std::fmax(std::nearbyint(ir), -32768.0), 32767.0), wq = std::fmin(std::fmax(std::nearbyint(qr), -32768.0), 32767.0);
        if (std::fabs(lo16(r) - wi) > 1.0 || std::fabs(hi16(r) - wq) > 1.0) off++;
        sat_hits += (std::fabs(ir) > 32768.5) + (std::fabs(qr) > 32768.5);
      }
  const uint32_t diag = tune_pair(word(32767, 32767), tune_phasor(tab.data(), 1u << 29));     // 45 degrees: Q' = 46339
  const uint32_t ndiag = tune_pair(word(-32768, -32768), tune_phasor(tab.data(), 1u << 29));  // Q' = -46341
  printf("saturation: %d saturated rails, %d off by more than one count; 45 degrees: (%d, %d) (%d, %d)\n", sat_hits, off,
         lo16(diag), hi16(diag), lo16(ndiag), hi16(ndiag));
  if (off || sat_hits < 1000 || hi16(diag) != 32767 || hi16(ndiag) != -32768 || std::abs(lo16(diag)) > 1 || std::abs(lo16(ndiag)) > 1) {
    printf("FAIL saturation\n");
    fails++;
  }

  // 5. the accumulator after calls of various sizes is the closed form, and each sample's phase is ph0 + t dphi
  const double stations[] = {0.0, 5000.0, -8000.0, 21999.5, -22049.0, 8390.0, 6890.0};
  const float offsets[] = {8390.0f, 5390.0f, 7390.0f, 6390.0f, 6890.0f};
  const int sizes[] = {1, 7, 64, 3, 128, 2, 5, 31};
  for (double s : stations)
    for (float o : offsets) {
      const uint32_t dphi = tune_dphi(o, s);
      const long long want = llround(((double)o - s) * 4294967296.0 / 44100.0);
      if (dphi != (uint32_t)(unsigned long long)want) { printf("FAIL dphi %g %g\n", (double)o, s); fails++; }
      uint32_t acc = 0, serial = 0;
      uint64_t total = 0;
      for (int c = 0; c < 40; c++) {
        const uint32_t n = 128u * (uint32_t)sizes[c % 8];
        for (uint32_t t = 0; t < n; t++, serial += dphi)
          if (tune_phase(acc, dphi, t) != serial) { printf("FAIL phase of sample %u of call %d\n", t, c); fails++; break; }
        acc = tune_phase(acc, dphi, n);
        total += n;
        if (acc != serial || acc != (uint32_t)(total * (uint64_t)dphi)) { printf("FAIL accumulator after call %d\n", c); fails++; break; }
      }
    }

  // 6. the sign: a tone at the station comes out at the tuning offset (USB: 5390 Hz) -- its phase advances by 5390 Hz
  {
    const double s = 5000.0;
    const uint32_t dphi = tune_dphi(5390.0f, s);
    double step = 0.0;
    for (uint32_t t = 0; t < 64; t++) {
      auto at = [&](uint32_t u) {
        const double a = 2.0 * M_PI * s * u / 44100.0;
        const uint32_t r = tune_pair(word((int)std::lround(20000 * std::cos(a)), (int)std::lround(20000 * std::sin(a))), tune_phasor(tab.data(), tune_phase(0u, dphi, u)));
        return std::atan2((double)hi16(r), (double)lo16(r));
      };
      double d = at(t + 1) - at(t);
      while (d < -M_PI) d += 2 * M_PI;
      while (d > M_PI) d -= 2 * M_PI;
      step += d / 64.0;
    }
    const double hz = step * 44100.0 / (2.0 * M_PI);
    printf("a tone at +5000 Hz tuned for USB comes out at %.2f Hz\n", hz);
    if (std::fabs(hz - 5390.0) > 1.0) { printf("FAIL sign\n"); fails++; }
  }
  if (fails) return 1;
  printf("OK\n");
  return 0;
}

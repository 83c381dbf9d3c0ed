// Host restatement of rdsp_engine_t's decimating pass (csrc/rdsp_tune.h, compiled here with -ffp-contract=off as the kernel
// is): the prototype's taps, a receiver's translated taps, the chain of fmaf, the rotation and requantization.
//   host_ddc_check            the checks below; prints OK
//   host_ddc_check rows DIR   reads DIR/params.bin (uint32: D, n_out, n_rx, then n_rx x {dphi, phase}), DIR/gain.bin (one
//                             float32), DIR/src.bin (uint32 words: 15 D pairs of history, then n_out D pairs), DIR/to.bin
//                             (float32) and DIR/station.bin (float64); writes DIR/out.bin ([n_rx][n_out] words: ddc_output of
//                             every receiver at phase + m D dphi), DIR/taps.bin (ddc_taps(D, gain)), DIR/g.bin ([n_rx][16 D]
//                             float pairs) and DIR/dphi.bin (ddc_dphi of each offset / station pair at D)
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
  if (par.size() < 3 || gb.size() != 4) { fprintf(stderr, "sizes\n"); return 2; }
  memcpy(&gain, gb.data(), 4);
  const int D = (int)par[0], T = DDC_TAPS_PER_PHASE * D;
  const size_t n_out = par[1], n_rx = par[2], m_st = to.size() / 4;
  if (D < 1 || D > DDC_MAX_D || par.size() != 3 + 2 * n_rx || src.size() != (size_t)DDC_HIST_PER_PHASE * D + n_out * D || st.size() != 8 * m_st) {
    fprintf(stderr, "sizes\n");
    return 2;
  }
  std::vector<float> h((size_t)T);
  ddc_taps(D, (double)gain, h.data());
  std::vector<float2> g(n_rx * (size_t)T);
  std::vector<uint32_t> out(n_rx * n_out), dphi(m_st);
  for (size_t r = 0; r < n_rx; r++) {
    const uint32_t dp = par[3 + 2 * r], ph0 = par[4 + 2 * r];
    float2 *gr = g.data() + r * (size_t)T;
    for (int k = 0; k < T; k++) gr[k] = ddc_tap(tab, h[(size_t)k], dp, (uint32_t)k);
    for (size_t m = 0; m < n_out; m++) /* x[0] is word 15 D of src: the newest of output m is x[(m + 1) D - 1] */
      out[r * n_out + m] = ddc_output(gr, T, src.data() + (size_t)DDC_HIST_PER_PHASE * D + (m + 1) * D - 1,
                                      tune_phasor(tab, tune_phase(ph0, (uint32_t)D * dp, (uint32_t)m)));
  }
  for (size_t k = 0; k < m_st; k++) {
    float o;
    double s;
    memcpy(&o, &to[4 * k], 4);
    memcpy(&s, &st[8 * k], 8);
    dphi[k] = ddc_dphi(o, s, D);
  }
  spill(d + "/out.bin", out.data(), out.size() * 4);
  spill(d + "/taps.bin", h.data(), h.size() * 4);
  spill(d + "/g.bin", g.data(), g.size() * sizeof(float2));
  spill(d + "/dphi.bin", dphi.data(), dphi.size() * 4);
  printf("OK D %d, %zu receivers x %zu outputs\n", D, n_rx, n_out);
  return 0;
}

int main(int argc, char **argv) {
  std::vector<float4> tab(TUNE_N);
  tune_table(tab.data());
  if (argc == 3 && std::string(argv[1]) == "rows") return rows(argv[2], tab.data());
  int fails = 0;

  // 1. the prototype: symmetric bit for bit, sum gain within the rounding of T floats, for every D and two gains; the sine
  //    series against libm's sin, the Bessel series against the tabulated I0(9)
  for (int D = 1; D <= DDC_MAX_D; D++)
    for (double gain : {1.0, 37.5}) {
      const int T = DDC_TAPS_PER_PHASE * D;
      std::vector<float> h((size_t)T);
      ddc_taps(D, gain, h.data());
      double sum = 0.0;
      for (int k = 0; k < T; k++) {
        sum += (double)h[(size_t)k];
        if (h[(size_t)k] != h[(size_t)(T - 1 - k)]) { printf("FAIL D %d: tap %d is not tap %d\n", D, k, T - 1 - k); fails++; break; }
      }
      if (std::fabs(sum / gain - 1.0) > T * std::ldexp(1.0, -25)) { printf("FAIL D %d: taps sum to %.9g x gain\n", D, sum / gain); fails++; }
    }
  double worst = 0.0;
  for (int D : {1, 2, 3, 7, 16, 64})
    for (int q = 0; q <= 40 * D; q++) worst = std::fmax(worst, std::fabs(ddc_sin_halfpi(q, D) - std::sin(M_PI * q / (2.0 * D))));
  printf("sine series: max abs err %.3e against libm\n", worst);
  if (!(worst < 1e-14)) { printf("FAIL sine series\n"); fails++; }
  // I0(9) = 1093.588354511375 (Abramowitz & Stegun 9.8; e^-9 I0(9) = 0.13495953), I0(0) = 1
  if (std::fabs(ddc_i0(9.0) / 1093.588354511375 - 1.0) > 1e-13 || ddc_i0(0.0) != 1.0) { printf("FAIL I0: %.17g\n", ddc_i0(9.0)); fails++; }

  // 2. the step at D, and D = 1 is tune_dphi
  const double stations[] = {0.0, 200000.0, -8000.0, 1411199.5, -22049.0, 8390.0};
  const float offsets[] = {8390.0f, 5390.0f, 7390.0f, 6390.0f, 6890.0f};
  for (double s : stations)
    for (float o : offsets)
      for (int D : {1, 2, 5, 16, 64}) {
        const long long want = llround(((double)o - s) * 4294967296.0 / (D * 44100.0));
        if (ddc_dphi(o, s, D) != (uint32_t)(unsigned long long)want) { printf("FAIL dphi %g %g %d\n", (double)o, s, D); fails++; }
        if (D == 1 && std::fabs(s) < 22050.0 && ddc_dphi(o, s, 1) != tune_dphi(o, s)) { printf("FAIL dphi at D = 1\n"); fails++; }
      }

  // 3. a constant source through a receiver at shift 0 comes out as the constant times the taps' sum (the DC gain)
  {
    const int D = 4, T = DDC_TAPS_PER_PHASE * D;
    std::vector<float> h((size_t)T);
    ddc_taps(D, 2.0, h.data());
    std::vector<float2> g((size_t)T);
    for (int k = 0; k < T; k++) g[(size_t)k] = ddc_tap(tab.data(), h[(size_t)k], 0u, (uint32_t)k);
    std::vector<uint32_t> x((size_t)T, (uint32_t)(uint16_t)(int16_t)1000 | (uint32_t)(uint16_t)(int16_t)-3000 << 16);
    const uint32_t y = ddc_output(g.data(), T, x.data() + T - 1, tune_phasor(tab.data(), 0u));
    if ((int16_t)(uint16_t)(y & 0xffffu) != 2000 || (int16_t)(uint16_t)(y >> 16) != -6000) { printf("FAIL DC gain: %08x\n", y); fails++; }
  }
  if (fails) return 1;
  printf("OK\n");
  return 0;
}

// Host restatement of rdsp_engine_t's three source passes on rows of any sample format (csrc/rdsp_tune.h, compiled here with
// -ffp-contract=off as the kernels are): the phasor table, src_value / src_pair, the rotation and requantization, the phase
// accumulator, the prototype's taps, the schedule, the chains of fmaf (tune_pair, ddc_output, rate_output).
//   host_source_pass_check check        the numbered checks below; prints OK last
//   host_source_pass_check values       prints "u8 B BITS" and "s8 B BITS" for all 256 bytes B and "f32 IN OUT" for a list of
//                                       floats (BITS, IN, OUT: the float's bit pattern in hex)
//   host_source_pass_check vectors DIR  reads DIR/words.bin, DIR/phases.bin (uint32 each), DIR/to.bin (float32), DIR/station.bin
//                                       (float64); writes DIR/tuned.bin (tune_pair of each word at its phase), DIR/dphi.bin
//                                       (the step of each offset / station pair at 44 100 Hz: rate_dphi at 1 / 1, which is
//                                       tune_dphi) and DIR/table.bin (the [1024][4] float table)
//   host_source_pass_check sched DIR    reads DIR/params.bin (uint32: P, Q, frac, n_out); writes DIR/sched.bin ([n_out] {n, r})
//                                       and DIR/pairs.bin (uint64: rate_pairs, rate_frac_after)
//   host_source_pass_check rows DIR     reads DIR/params.bin (uint32: format, pass (0 tune, 1 decimating, 2 polyphase), P, Q,
//                                       frac, n_out, n_rx, then n_rx x {dphi, phase}), DIR/gain.bin (one float32), DIR/hist.bin
//                                       (float32 pairs: the VALUES of the pairs before the call, rate_keep(P, Q) of them),
//                                       DIR/src.bin (the call's pairs in the format's own elements), DIR/to.bin (float32) and
//                                       DIR/station.bin (float64); writes DIR/out.bin ([n_rx][n_out] words I | Q << 16 of
//                                       tune_pair, ddc_output or rate_output), DIR/dphi.bin (rate_dphi of each offset / station
//                                       pair at P / Q) and, with a filter, DIR/taps.bin (rate_taps(P, Q, gain)), DIR/g.bin
//                                       (pass 1: [n_rx][16 D] float pairs) and DIR/sched.bin (pass 2: [n_out] {n, r})
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
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
static uint32_t bits_of(float v) {
  uint32_t u;
  memcpy(&u, &v, 4);
  return u;
}
/* DIR/to.bin and DIR/station.bin -> the step of each offset / station pair at P / Q */
static bool steps_of(const std::string &d, int P, int Q, std::vector<uint32_t> &dphi) {
  std::vector<char> to = slurp(d + "/to.bin"), st = slurp(d + "/station.bin");
  const size_t m = to.size() / 4;
  if (st.size() != 8 * m) return false;
  dphi.resize(m);
  for (size_t k = 0; k < m; k++) {
    float o;
    double s;
    memcpy(&o, &to[4 * k], 4);
    memcpy(&s, &st[8 * k], 8);
    dphi[k] = rate_dphi(o, s, P, Q); /* Q = 1: ddc_dphi(o, s, P); P = Q = 1: tune_dphi(o, s) */
  }
  return true;
}

static int values() {
  for (uint32_t b = 0; b < 256; b++) printf("u8 %u %08x\n", b, bits_of(src_value(SRC_U8, b)));
  for (uint32_t b = 0; b < 256; b++) printf("s8 %u %08x\n", b, bits_of(src_value(SRC_S8, b)));
  const float inf = std::numeric_limits<float>::infinity();
  const float list[] = {0.0f, 1.0f, -1.0f, 0x1p-15f, -0x1p-15f, 0x1p-140f, 0.99999994f, 256.0f, -256.0f, 256.5f, -256.5f, 3e38f, -3e38f,
                        inf, -inf, std::numeric_limits<float>::quiet_NaN()};
  for (float x : list) printf("f32 %08x %08x\n", bits_of(x), bits_of(src_value(SRC_F32, bits_of(x))));
  return 0;
}

static int vectors(const std::string &d, const float4 *tab) {
  std::vector<char> w = slurp(d + "/words.bin"), p = slurp(d + "/phases.bin");
  const size_t n = w.size() / 4;
  std::vector<uint32_t> out(n), dphi;
  if (p.size() != w.size() || !steps_of(d, 1, 1, dphi)) { fprintf(stderr, "sizes\n"); return 2; }
  for (size_t k = 0; k < n; k++) {
    uint32_t wk, pk;
    memcpy(&wk, &w[4 * k], 4);
    memcpy(&pk, &p[4 * k], 4);
    out[k] = tune_pair(wk, tune_phasor(tab, pk));
  }
  spill(d + "/tuned.bin", out.data(), n * 4);
  spill(d + "/dphi.bin", dphi.data(), dphi.size() * 4);
  spill(d + "/table.bin", tab, TUNE_N * sizeof(float4));
  printf("OK %zu words, %zu steps\n", n, dphi.size());
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

template <int F>
static void pairs_of(const std::vector<char> &raw, std::vector<float2> &x) {
  const size_t n = raw.size() / (size_t)src_pair_bytes(F);
  std::vector<uint64_t> aligned((raw.size() + 7) / 8 + 1); /* a float pair is read as one 8-byte element */
  memcpy(aligned.data(), raw.data(), raw.size());
  for (size_t i = 0; i < n; i++) x.push_back(src_pair<F>(aligned.data(), (long long)i));
}

static int rows(const std::string &d, const float4 *tab) {
  std::vector<char> pb = slurp(d + "/params.bin"), gb = slurp(d + "/gain.bin"), hb = slurp(d + "/hist.bin"), sb = slurp(d + "/src.bin");
  std::vector<uint32_t> par(pb.size() / 4);
  memcpy(par.data(), pb.data(), par.size() * 4);
  float gain;
  if (par.size() < 7 || gb.size() != 4 || par.size() != 7 + 2 * (size_t)par[6]) { fprintf(stderr, "sizes\n"); return 2; }
  memcpy(&gain, gb.data(), 4);
  const int fmt = (int)par[0], pass = (int)par[1];
  int P = (int)par[2], Q = (int)par[3];
  const uint32_t frac = par[4];
  const size_t n_out = par[5], n_rx = par[6];
  if (fmt < 0 || fmt >= SRC_FORMATS || pass < 0 || pass > 2 || sb.size() % (size_t)src_pair_bytes(fmt) != 0 || hb.size() % 8 != 0) { fprintf(stderr, "format\n"); return 2; }
  if (!rate_reduce(P, Q) || P != (int)par[2] || frac >= (uint32_t)Q || pass != (Q > 1 ? 2 : P > 1 ? 1 : 0)) { fprintf(stderr, "rate\n"); return 2; }
  std::vector<float2> x(hb.size() / 8);
  memcpy(x.data(), hb.data(), hb.size());
  const size_t keep = x.size();
  switch (fmt) {
    case SRC_S16: pairs_of<SRC_S16>(sb, x); break;
    case SRC_U8: pairs_of<SRC_U8>(sb, x); break;
    case SRC_S8: pairs_of<SRC_S8>(sb, x); break;
    default: pairs_of<SRC_F32>(sb, x); break;
  }
  const size_t pairs = x.size() - keep;
  if (keep != (size_t)rate_keep(P, Q) || pairs != (size_t)rate_pairs(frac, P, Q, (uint32_t)n_out)) { fprintf(stderr, "sizes of pass %d\n", pass); return 2; }
  std::vector<uint32_t> out(n_rx * n_out), dphi;
  if (!steps_of(d, P, Q, dphi)) { fprintf(stderr, "sizes\n"); return 2; }
  const int Tb = rate_tb(P, Q), Dc = rate_dc(P, Q); /* pass 1: T = 16 D = Tb */
  std::vector<float> h((size_t)Tb * Q);
  if (pass) rate_taps(P, Q, (double)gain, h.data());
  if (pass == 0) {
    for (size_t r = 0; r < n_rx; r++)
      for (size_t t = 0; t < n_out; t++)
        out[r * n_out + t] = tune_pair(x[t], tune_phasor(tab, tune_phase(par[8 + 2 * r], par[7 + 2 * r], (uint32_t)t)));
  } else if (pass == 1) {
    const int D = P, T = DDC_TAPS_PER_PHASE * D;
    std::vector<float2> g(n_rx * (size_t)T);
    for (size_t r = 0; r < n_rx; r++) {
      const uint32_t dp = par[7 + 2 * r], ph0 = par[8 + 2 * r];
      float2 *gr = g.data() + r * (size_t)T;
      for (int k = 0; k < T; k++) gr[k] = ddc_tap(tab, h[(size_t)k], dp, (uint32_t)k);
      for (size_t m = 0; m < n_out; m++) /* the newest pair of output m is pair (m + 1) D - 1 of the call */
        out[r * n_out + m] = ddc_output(gr, T, x.data() + keep + (m + 1) * (size_t)D - 1, tune_phasor(tab, tune_phase(ph0, (uint32_t)D * dp, (uint32_t)m)));
    }
    spill(d + "/g.bin", g.data(), g.size() * sizeof(float2));
  } else {
    std::vector<float> hbr((size_t)Tb);
    std::vector<RateStep> sc(n_out);
    for (size_t i = 0; i < n_out; i++) {
      const RateStep s = sc[i] = rate_step(frac, P, Q, (uint32_t)i);
      if (s.n < 0 || (size_t)s.n >= pairs || s.r < 0 || s.r >= Q) { fprintf(stderr, "schedule\n"); return 2; }
      for (int j = 0; j < Tb; j++) hbr[(size_t)j] = h[(size_t)j * Q + s.r];
      for (size_t r = 0; r < n_rx; r++) {
        const uint32_t dp = par[7 + 2 * r], ph0 = par[8 + 2 * r];
        out[r * n_out + i] = rate_output(tab, hbr.data(), Tb, dp, x.data() + keep + s.n, tune_phasor(tab, rate_phase(ph0, dp, s.n, Dc)));
      }
    }
    spill(d + "/sched.bin", sc.data(), sc.size() * sizeof(RateStep));
  }
  spill(d + "/out.bin", out.data(), out.size() * 4);
  spill(d + "/dphi.bin", dphi.data(), dphi.size() * 4);
  if (pass) spill(d + "/taps.bin", h.data(), h.size() * 4);
  printf("OK format %d, pass %d, %d / %d, %zu receivers x %zu outputs from %zu pairs\n", fmt, pass, P, Q, n_rx, n_out, pairs);
  return 0;
}

// ---- the tuning pass -------------------------------------------------------------------------------------------------------
static int check_tune(const float4 *tab) {
  int fails = 0;
  std::mt19937 rng(11);

  // 1. phase 0 is exactly (1, 0)
  const float2 one = tune_phasor(tab, 0u);
  if (!(one.x == 1.0f && one.y == 0.0f && !std::signbit(one.y))) { printf("FAIL phase 0 gives (%a, %a)\n", one.x, one.y); fails++; }

  // 2. the phasor against cos / sin in double: every 2^9-th phase, every phase around each table entry, random phases
  double worst = 0.0;
  auto probe = [&](uint32_t ph) {
    const float2 cs = tune_phasor(tab, ph);
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
    if (tune_pair(w, tune_phasor(tab, 0u)) != w) { printf("FAIL identity %08x\n", w); fails++; break; }
  }

  // 4. full-scale rotations saturate (never wrap): within one count of the saturated double rotation; the corners exactly
  int sat_hits = 0, off = 0;
  const int full[] = {-32768, 32767};
  for (int i : full)
    for (int q : full)
      for (uint32_t k = 0; k < 4096; k++) {
        const uint32_t ph = k * 1048573u;
        const float2 cs = tune_phasor(tab, ph);
        const uint32_t r = tune_pair(word(i, q), cs);
        const double a = 2.0 * M_PI * (double)ph / 4294967296.0;
        const double ir = i * std::cos(a) - q * std::sin(a), qr = q * std::cos(a) + i * std::sin(a);
        const double wi = std::fmin(std::fmax(std::nearbyint(ir), -32768.0), 32767.0), wq = std::fmin(std::fmax(std::nearbyint(qr), -32768.0), 32767.0);
        if (std::fabs(lo16(r) - wi) > 1.0 || std::fabs(hi16(r) - wq) > 1.0) off++;
        sat_hits += (std::fabs(ir) > 32768.5) + (std::fabs(qr) > 32768.5);
      }
  const uint32_t diag = tune_pair(word(32767, 32767), tune_phasor(tab, 1u << 29));     // 45 degrees: Q' = 46339
  const uint32_t ndiag = tune_pair(word(-32768, -32768), tune_phasor(tab, 1u << 29));  // Q' = -46341
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
        const uint32_t r = tune_pair(word((int)std::lround(20000 * std::cos(a)), (int)std::lround(20000 * std::sin(a))), tune_phasor(tab, tune_phase(0u, dphi, u)));
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
  return fails;
}

// ---- the decimating pass ---------------------------------------------------------------------------------------------------
static int check_ddc(const float4 *tab) {
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
    for (int k = 0; k < T; k++) g[(size_t)k] = ddc_tap(tab, h[(size_t)k], 0u, (uint32_t)k);
    std::vector<uint32_t> x((size_t)T, word(1000, -3000));
    const uint32_t y = ddc_output(g.data(), T, x.data() + T - 1, tune_phasor(tab, 0u));
    if (lo16(y) != 2000 || hi16(y) != -6000) { printf("FAIL DC gain: %08x\n", y); fails++; }
  }
  return fails;
}

// ---- the polyphase pass ----------------------------------------------------------------------------------------------------
static int check_rate(const float4 *tab) {
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
    std::vector<uint32_t> x((size_t)Tb, word(1000, -3000));
    for (int r : {0, 1, 73, 146}) {
      for (int j = 0; j < Tb; j++) hb[(size_t)j] = h[(size_t)j * Q + r];
      const uint32_t y = rate_output(tab, hb.data(), Tb, 0u, x.data() + Tb - 1, tune_phasor(tab, 0u));
      if (abs(lo16(y) - 2000) > 1 || abs(hi16(y) + 6000) > 1) { printf("FAIL DC gain of branch %d: %08x\n", r, y); fails++; }
    }
  }
  return fails;
}

int main(int argc, char **argv) {
  std::vector<float4> tab(TUNE_N);
  tune_table(tab.data());
  const std::string mode = argc > 1 ? argv[1] : "";
  if (argc == 2 && mode == "values") return values();
  if (argc == 3 && mode == "vectors") return vectors(argv[2], tab.data());
  if (argc == 3 && mode == "sched") return sched(argv[2]);
  if (argc == 3 && mode == "rows") return rows(argv[2], tab.data());
  if (argc != 2 || mode != "check") {
    fprintf(stderr, "usage: host_source_pass_check check | values | vectors DIR | sched DIR | rows DIR\n");
    return 2;
  }
  if (check_tune(tab.data()) + check_ddc(tab.data()) + check_rate(tab.data())) return 1;
  printf("OK\n");
  return 0;
}

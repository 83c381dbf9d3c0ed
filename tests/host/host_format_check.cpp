// Host restatement of rdsp_engine_t's three source passes on rows of any sample format (csrc/rdsp_tune.h, compiled here with
// -ffp-contract=off as the kernels are): src_value / src_pair give the value of every element, and everything after it is the
// header's arithmetic on values (tune_pair, ddc_output, rate_output).
//   host_format_check values     prints "u8 B BITS" and "s8 B BITS" for all 256 bytes B and "f32 IN OUT" for a list of floats
//                                (BITS, IN, OUT: the float's bit pattern in hex)
//   host_format_check rows DIR   reads DIR/params.bin (uint32: format, pass (0 tune, 1 decimating, 2 polyphase), P, Q, frac,
//                                n_out, n_rx, then n_rx x {dphi, phase}), DIR/gain.bin (one float32), DIR/hist.bin (float32
//                                pairs: the VALUES of the pairs before the call, 15 D or Tb of them, none for pass 0) and
//                                DIR/src.bin (the call's pairs in the format's own elements); writes DIR/out.bin ([n_rx][n_out]
//                                words I | Q << 16)
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
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
static uint32_t bits_of(float v) {
  uint32_t u;
  memcpy(&u, &v, 4);
  return u;
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
  std::vector<uint32_t> out(n_rx * n_out);
  if (pass == 0) {
    if (keep != 0 || pairs != n_out) { fprintf(stderr, "sizes of the tuning pass\n"); return 2; }
    for (size_t r = 0; r < n_rx; r++)
      for (size_t t = 0; t < n_out; t++)
        out[r * n_out + t] = tune_pair(x[t], tune_phasor(tab, tune_phase(par[8 + 2 * r], par[7 + 2 * r], (uint32_t)t)));
  } else if (pass == 1) {
    const int D = P, T = DDC_TAPS_PER_PHASE * D;
    if (Q != 1 || D < 2 || D > DDC_MAX_D || keep != (size_t)(DDC_HIST_PER_PHASE * D) || pairs != n_out * (size_t)D) { fprintf(stderr, "sizes of the decimating pass\n"); return 2; }
    std::vector<float> h((size_t)T);
    ddc_taps(D, (double)gain, h.data());
    std::vector<float2> g((size_t)T);
    for (size_t r = 0; r < n_rx; r++) {
      const uint32_t dp = par[7 + 2 * r], ph0 = par[8 + 2 * r];
      for (int k = 0; k < T; k++) g[(size_t)k] = ddc_tap(tab, h[(size_t)k], dp, (uint32_t)k);
      for (size_t m = 0; m < n_out; m++)
        out[r * n_out + m] = ddc_output(g.data(), T, x.data() + keep + (m + 1) * (size_t)D - 1, tune_phasor(tab, tune_phase(ph0, (uint32_t)D * dp, (uint32_t)m)));
    }
  } else {
    if (!rate_reduce(P, Q) || P != (int)par[2] || Q < 2 || frac >= (uint32_t)Q) { fprintf(stderr, "rate\n"); return 2; }
    const int Tb = rate_tb(P, Q), Dc = rate_dc(P, Q);
    if (keep != (size_t)Tb || pairs != (size_t)rate_pairs(frac, P, Q, (uint32_t)n_out)) { fprintf(stderr, "sizes of the polyphase pass\n"); return 2; }
    std::vector<float> h((size_t)Tb * Q), hbr((size_t)Tb);
    rate_taps(P, Q, (double)gain, h.data());
    for (size_t i = 0; i < n_out; i++) {
      const RateStep s = rate_step(frac, P, Q, (uint32_t)i);
      if (s.n < 0 || (size_t)s.n >= pairs) { fprintf(stderr, "schedule\n"); return 2; }
      for (int j = 0; j < Tb; j++) hbr[(size_t)j] = h[(size_t)j * Q + s.r];
      for (size_t r = 0; r < n_rx; r++) {
        const uint32_t dp = par[7 + 2 * r], ph0 = par[8 + 2 * r];
        out[r * n_out + i] = rate_output(tab, hbr.data(), Tb, dp, x.data() + keep + s.n, tune_phasor(tab, rate_phase(ph0, dp, s.n, Dc)));
      }
    }
  }
  spill(d + "/out.bin", out.data(), out.size() * 4);
  printf("OK format %d, pass %d, %zu receivers x %zu outputs from %zu pairs\n", fmt, pass, n_rx, n_out, pairs);
  return 0;
}

int main(int argc, char **argv) {
  std::vector<float4> tab(TUNE_N);
  tune_table(tab.data());
  if (argc == 2 && std::string(argv[1]) == "values") return values();
  if (argc == 3 && std::string(argv[1]) == "rows") return rows(argv[2], tab.data());
  fprintf(stderr, "usage: host_format_check values | rows DIR\n");
  return 2;
}

/*
 * host_fm_check.cpp -- csrc/rdsp_fm.h, the arithmetic of rdsp_engine_t's narrow-band FM detector, as a program of its own: plain
 * and with -fsanitize=address,undefined.
 *
 *   host_fm_check atan2
 *     fm_atan2 against the double atan2 over every t = j / 2^20 (y = t, x = 1, and the seven other octants of it) and over a
 *     million drawn pairs of every scale; the special cases (both zero, signed zeros, the axes, the diagonals, huge with tiny).
 *     Prints "worst fm_atan2 error E rad" and fails above 2^-19.
 *   host_fm_check IN OUT W deviation_hz tau_us n_rows n_blocks call_blocks
 *     IN: int16 [n_rows][n_blocks * 128][2], the IQ pairs of every row's stream.  Every row starts from a fresh channel's state
 *     (zeros) and runs through fm_reference in calls of call_blocks blocks (the last one shorter), the state handed from call to
 *     call; then once more in ONE call, which must give the same bits in every output and every state word.  OUT: 32-bit words
 *     -- the 16 W taps, k, a, then per row [n] y, [n] lvl, [50] state words as the last call left them.
 * Buffers are exactly sized heap allocations (a call's words are copied into one of their own: a read past the call shows).
 * Prints "host_fm_check OK".
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "rdsp_fm.h"

using namespace rdsp_fm;

static double worst = 0.0;
static int check_pair(float y, float x) {
  const float got = fm_atan2(y, x);
  const double want = atan2((double)y, (double)x), err = fabs((double)got - want);
  if (!(err <= 1.9073486328125e-06)) { printf("FAIL: fm_atan2(%a, %a) = %a, atan2 %.17g\n", (double)y, (double)x, (double)got, want); return 0; }
  worst = std::max(worst, err);
  return 1;
}
static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t draw() { /* xorshift64* */
  rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
  return (uint32_t)((rng_state * 0x2545F4914F6CDD1Dull) >> 32);
}
static float bits(uint32_t b) { float f; memcpy(&f, &b, 4); return f; }
static uint32_t word(float f) { uint32_t b; memcpy(&b, &f, 4); return b; }

static int atan2_holds() {
  for (uint32_t j = 0; j <= (1u << 20); j++) {
    const float t = (float)j * 9.5367431640625e-07f;
    for (int o = 0; o < 8; o++) {
      const float a = (o & 1) ? 1.0f : t, b = (o & 1) ? t : 1.0f;
      if (!check_pair((o & 2) ? -a : a, (o & 4) ? -b : b)) return 0;
    }
  }
  for (int i = 0; i < 1000000; i++) { /* any sign, exponents 2^-60 ... 2^60: the products of int16 counts lie well inside */
    const uint32_t a = draw(), b = draw();
    const float y = bits((a & 0x807fffffu) | ((67u + (a >> 23) % 121u) << 23)), x = bits((b & 0x807fffffu) | ((67u + (b >> 23) % 121u) << 23));
    if (!check_pair(y, x)) return 0;
  }
  /* both zero: +0 whatever the signs; one zero: the axes, with the sign of y (also of a y = -0) */
  const float z[2] = {0.0f, -0.0f};
  for (int i = 0; i < 2; i++)
    for (int j = 0; j < 2; j++)
      if (word(fm_atan2(z[i], z[j])) != 0u) { printf("FAIL: fm_atan2(+-0, +-0)\n"); return 0; }
  if (word(fm_atan2(0.0f, 2.0f)) != 0u || word(fm_atan2(-0.0f, 2.0f)) != 0x80000000u || fm_atan2(0.0f, -2.0f) != FM_PI || fm_atan2(-0.0f, -2.0f) != -FM_PI ||
      fm_atan2(3.0f, 0.0f) != FM_PI_2 || fm_atan2(-3.0f, -0.0f) != -FM_PI_2) { printf("FAIL: fm_atan2 on the axes\n"); return 0; }
  const float huge = 3.0e38f, tiny = 1.0e-44f; /* a subnormal */
  const float pairs[][2] = {{1.0f, 1.0f}, {1.0f, -1.0f}, {-1.0f, 1.0f}, {-1.0f, -1.0f}, {huge, huge}, {tiny, tiny}, {-tiny, tiny},
                            {huge, tiny}, {tiny, huge}, {-tiny, -huge}, {-huge, -tiny}, {huge, -tiny}, {tiny, -huge}};
  for (const auto &q : pairs)
    if (!check_pair(q[0], q[1])) return 0;
  printf("worst fm_atan2 error %.3e rad (bound %.3e)\n", worst, 1.9073486328125e-06);
  return 1;
}

int main(int argc, char **argv) {
  if (argc == 2 && strcmp(argv[1], "atan2") == 0) {
    if (!atan2_holds()) return 1;
    printf("host_fm_check OK\n");
    return 0;
  }
  if (argc != 9) { printf("usage: host_fm_check atan2 | IN OUT W deviation_hz tau_us n_rows n_blocks call_blocks\n"); return 1; }
  const int W = atoi(argv[3]);
  const float deviation = (float)atof(argv[4]), tau = (float)atof(argv[5]);
  const size_t n_rows = (size_t)atol(argv[6]), n_blocks = (size_t)atol(argv[7]), call_blocks = (size_t)atol(argv[8]);
  if (!width_ok(W) || !deviation_ok(deviation) || !tau_ok(tau) || call_blocks < 1) return 2;
  const size_t n = n_blocks * BLOCK, T = (size_t)(TAPS_PER_W * W), per_row = 2 * n + FM_STATE_WORDS;
  std::vector<int16_t> in(n_rows * n * 2);
  std::vector<float> h(T), y(n), lvl(n), y_one(n), lvl_one(n);
  std::vector<uint32_t> out(T + 2 + n_rows * per_row);
  FILE *f = fopen(argv[1], "rb");
  if (!f || fread(in.data(), 2, in.size(), f) != in.size()) { printf("FAIL: cannot read %s\n", argv[1]); return 1; }
  fclose(f);
  fm_taps(W, h.data());
  const float k = fm_scale(deviation), a = fm_deemph_a(tau);
  const int deemph = tau != 0.0f;
  for (size_t i = 0; i < T; i++) out[i] = word(h[i]);
  out[T] = word(k); out[T + 1] = word(a);
  for (size_t r = 0; r < n_rows; r++) {
    std::vector<uint32_t> x(n), state(FM_STATE_WORDS, 0u), state_one(FM_STATE_WORDS, 0u);
    for (size_t i = 0; i < n; i++) x[i] = (uint32_t)(uint16_t)in[(r * n + i) * 2] | ((uint32_t)(uint16_t)in[(r * n + i) * 2 + 1] << 16);
    for (size_t b = 0; b < n_blocks; b += call_blocks) {
      const size_t nb = std::min(call_blocks, n_blocks - b);
      std::vector<uint32_t> call(x.begin() + (long)(b * BLOCK), x.begin() + (long)((b + nb) * BLOCK));
      std::vector<float> cy(nb * BLOCK), cl(nb * BLOCK);
      fm_reference(h.data(), W, k, a, deemph, state.data(), call.data(), (int)(nb * BLOCK), cy.data(), cl.data());
      std::copy(cy.begin(), cy.end(), y.begin() + (long)(b * BLOCK));
      std::copy(cl.begin(), cl.end(), lvl.begin() + (long)(b * BLOCK));
    }
    fm_reference(h.data(), W, k, a, deemph, state_one.data(), x.data(), (int)n, y_one.data(), lvl_one.data());
    if (memcmp(y.data(), y_one.data(), n * 4) != 0 || memcmp(lvl.data(), lvl_one.data(), n * 4) != 0 || state != state_one) {
      printf("FAIL: row %zu in calls of %zu blocks is not the row in one call\n", r, call_blocks);
      return 1;
    }
    uint32_t *o = out.data() + T + 2 + r * per_row;
    memcpy(o, y.data(), n * 4);
    memcpy(o + n, lvl.data(), n * 4);
    memcpy(o + 2 * n, state.data(), FM_STATE_WORDS * 4);
  }
  f = fopen(argv[2], "wb");
  if (!f || fwrite(out.data(), 4, out.size(), f) != out.size()) { printf("FAIL: cannot write %s\n", argv[2]); return 1; }
  fclose(f);
  printf("host_fm_check OK\n");
  return 0;
}

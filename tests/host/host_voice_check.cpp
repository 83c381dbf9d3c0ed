/*
 * host_voice_check.cpp -- csrc/rdsp_voice.h, the arithmetic of rdsp_engine_t's voice-rate audio, as a program of its own: plain
 * and with -fsanitize=address,undefined.
 *
 *   host_voice_check IN OUT R n_rows n_blocks call_blocks
 *
 * IN: int16 [n_rows][n_blocks * 128], the left words of every row's stream.  Every row starts from a fresh engine's history
 * (zeros) and runs through voice_reference in calls of call_blocks blocks (the last one shorter), the history handed from
 * call to call.  OUT: int32 words -- the 16 R taps, then [n_rows][n_blocks * 128 / R] outputs, then [n_rows][60] histories as
 * the last call left them.  Every output is computed a second time in the kernel's form -- the tap words of voice_tap_pairs,
 * two 16-bit products a word into the int32 sums of the hi and the lo parts, which may not leave int32 -- and must be the same.
 * On the way voice_round_sat is held to its definition at the ties, the floor and the clamps, and
 * R other than 2 and 4 is refused.  Buffers are exactly sized heap allocations.  Prints "host_voice_check OK".
 */
#include <limits.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "rdsp_voice.h"

using namespace rdsp_voice;

static int rounding_holds() {
  const int64_t half = (int64_t)1 << 17, one = (int64_t)1 << 18;
  int ok = voice_round_sat(0) == 0 && voice_round_sat(half - 1) == 0 && voice_round_sat(half) == 1 && voice_round_sat(-half) == 0 &&
           voice_round_sat(-half - 1) == -1 && voice_round_sat(one + half) == 2 && voice_round_sat(-one - half) == -1 &&
           voice_round_sat(-one - half - 1) == -2 && voice_round_sat(-1) == 0 && voice_round_sat(-one) == -1;
  ok = ok && voice_round_sat(32767 * one + half - 1) == 32767 && voice_round_sat(32767 * one + half) == 32767 &&
       voice_round_sat(-32768 * one - half) == -32768 && voice_round_sat(-32768 * one - half - 1) == -32768 &&
       voice_round_sat(((int64_t)1 << 34) - 1) == 32767 && voice_round_sat(-((int64_t)1 << 34)) == -32768;
  return ok && rate_ok(2) && rate_ok(4) && !rate_ok(0) && !rate_ok(1) && !rate_ok(3) && !rate_ok(8) && !rate_ok(-2);
}

/* output m of a row x (zeros in front of it) as the kernel sums it; -1 in *ok if a sum left int32 */
static int16_t pairs_output(const uint32_t *words, int R, const int16_t *x, long m, int *ok) {
  int64_t hi = 0, lo = 0;
  for (int a = 0; a < TAPS_PER_PHASE; a++)
    for (int pp = 0; pp < R / 2; pp++) {
      const uint32_t *w = words + ((size_t)a * (size_t)(R / 2) + (size_t)pp) * 2;
      for (int half = 0; half < 2; half++) {
        const long s = (long)R * (m - a) + 2 * pp + half;
        const int64_t v = s < 0 ? 0 : x[s];
        hi += v * (int16_t)(w[0] >> (16 * half));
        lo += v * (int16_t)(w[1] >> (16 * half));
        if (hi < INT32_MIN || hi > INT32_MAX || lo < INT32_MIN || lo > INT32_MAX) *ok = 0;
      }
    }
  return voice_round_sat(voice_acc_join((int32_t)hi, (int32_t)lo));
}

int main(int argc, char **argv) {
  if (!rounding_holds()) { printf("FAIL: voice_round_sat or rate_ok\n"); return 1; }
  if (argc != 7) { printf("usage: host_voice_check IN OUT R n_rows n_blocks call_blocks\n"); return 1; }
  const int R = atoi(argv[3]);
  const size_t n_rows = (size_t)atol(argv[4]), n_blocks = (size_t)atol(argv[5]), call_blocks = (size_t)atol(argv[6]);
  if (!rate_ok(R) || call_blocks < 1) return 2;
  const size_t n = n_blocks * BLOCK, n_out = n / (size_t)R, T = (size_t)(TAPS_PER_PHASE * R);
  std::vector<int16_t> in(n_rows * n), y(n_out);
  std::vector<int32_t> q(T), out(T + n_rows * n_out + n_rows * VOICE_HIST);
  FILE *f = fopen(argv[1], "rb");
  if (!f || fread(in.data(), 2, in.size(), f) != in.size()) { printf("FAIL: cannot read %s\n", argv[1]); return 1; }
  fclose(f);
  voice_taps(R, q.data());
  std::vector<uint32_t> words(T);
  voice_tap_pairs(R, q.data(), words.data());
  for (size_t k = 0; k < T; k++) {
    int32_t hi, lo;
    voice_tap_split(q[k], &hi, &lo);
    if (hi * 256 + lo != q[k] || lo < -128 || lo > 127 || hi < -32768 || hi > 32767) { printf("FAIL: voice_tap_split(%d)\n", (int)q[k]); return 1; }
  }
  std::copy(q.begin(), q.end(), out.begin());
  for (size_t r = 0; r < n_rows; r++) {
    std::vector<int32_t> hist(VOICE_HIST, 0);
    for (size_t b = 0; b < n_blocks; b += call_blocks) {
      const size_t nb = std::min(call_blocks, n_blocks - b);
      std::vector<int16_t> call(in.begin() + (long)(r * n + b * BLOCK), in.begin() + (long)(r * n + (b + nb) * BLOCK)); /* its own allocation: a read past the call shows */
      voice_reference(q.data(), R, hist.data(), call.data(), 1, (int)(nb * BLOCK), y.data() + b * BLOCK / (size_t)R);
    }
    for (size_t m = 0; m < n_out; m++) {
      int ok = 1;
      if (pairs_output(words.data(), R, &in[r * n], (long)m, &ok) != y[m] || !ok) { printf("FAIL: the kernel's form, row %zu output %zu\n", r, m); return 1; }
      out[T + r * n_out + m] = y[m];
    }
    std::copy(hist.begin(), hist.end(), out.begin() + (long)(T + n_rows * n_out + r * VOICE_HIST));
  }
  f = fopen(argv[2], "wb");
  if (!f || fwrite(out.data(), 4, out.size(), f) != out.size()) { printf("FAIL: cannot write %s\n", argv[2]); return 1; }
  fclose(f);
  printf("host_voice_check OK\n");
  return 0;
}

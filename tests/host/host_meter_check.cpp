/*
 * host_meter_check.cpp -- csrc/rdsp_meter.h, the arithmetic of rdsp_engine_t's signal meter and squelch, as a program of its
 * own: compiled with -ffp-contract=off as the kernel is, plain and with -fsanitize=address,undefined.
 *
 *   host_meter_check IN OUT n_rows n_blocks attack decay squelch open_ms close_ms hang_blocks
 *
 * IN: float32 [n_rows][n_blocks * 128], the demodulated rows.  Every row starts from the state of a fresh engine (level 0,
 * gate closed, hang 0) and runs its blocks in order.  OUT: [n_rows][n_blocks][5] words = ms, pk, level (float32), open, hang
 * (int32).  The setters' limits are checked on the way: a refused setting exits with 2.  Buffers are exactly sized heap
 * allocations.  Prints "host_meter_check OK".
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <limits>
#include <vector>

#include "rdsp_meter.h"

using namespace rdsp_meter;

static int limits_hold() {
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
  int ok = coefficients_ok(0.5f, 0.0625f) && coefficients_ok(1.0f, 1.0f) && !coefficients_ok(0.0f, 0.5f) && !coefficients_ok(0.5f, 0.0f) &&
           !coefficients_ok(1.5f, 0.5f) && !coefficients_ok(0.5f, -0.1f) && !coefficients_ok(nan, 0.5f) && !coefficients_ok(0.5f, nan);
  ok = ok && squelch_ok(0.0f, 0.0f, 0) && squelch_ok(1e-3f, 1e-4f, HANG_MAX) && !squelch_ok(1e-4f, 1e-3f, 0) && !squelch_ok(-1.0f, -2.0f, 0) &&
       !squelch_ok(nan, 0.0f, 0) && !squelch_ok(1.0f, nan, 0) && !squelch_ok(inf, 0.0f, 0) && !squelch_ok(1.0f, 0.5f, -1) &&
       !squelch_ok(1.0f, 0.5f, HANG_MAX + 1);
  return ok;
}

int main(int argc, char **argv) {
  if (!limits_hold()) { printf("FAIL: the setters' limits\n"); return 1; }
  if (argc != 11) { printf("usage: host_meter_check IN OUT n_rows n_blocks attack decay squelch open_ms close_ms hang_blocks\n"); return 1; }
  const size_t n_rows = (size_t)atol(argv[3]), n_blocks = (size_t)atol(argv[4]);
  MeterSet s;
  s.attack = strtof(argv[5], nullptr); s.decay = strtof(argv[6], nullptr); s.squelch = atoi(argv[7]);
  s.open_ms = strtof(argv[8], nullptr); s.close_ms = strtof(argv[9], nullptr); s.hang_blocks = atoi(argv[10]);
  if (!coefficients_ok(s.attack, s.decay) || (s.squelch && !squelch_ok(s.open_ms, s.close_ms, s.hang_blocks))) return 2;
  std::vector<float> in(n_rows * n_blocks * BLOCK);
  std::vector<uint32_t> out(n_rows * n_blocks * 5);
  FILE *f = fopen(argv[1], "rb");
  if (!f || fread(in.data(), 4, in.size(), f) != in.size()) { printf("FAIL: cannot read %s\n", argv[1]); return 1; }
  fclose(f);
  for (size_t r = 0; r < n_rows; r++) {
    MeterState g = {0.0f, 0, 0};
    for (size_t b = 0; b < n_blocks; b++) {
      float ms, pk;
      block_step(g, s, &in[(r * n_blocks + b) * BLOCK], &ms, &pk);
      uint32_t *o = &out[(r * n_blocks + b) * 5];
      memcpy(o, &ms, 4); memcpy(o + 1, &pk, 4); memcpy(o + 2, &g.level, 4);
      o[3] = (uint32_t)g.open; o[4] = (uint32_t)g.hang;
    }
  }
  f = fopen(argv[2], "wb");
  if (!f || fwrite(out.data(), 4, out.size(), f) != out.size()) { printf("FAIL: cannot write %s\n", argv[2]); return 1; }
  fclose(f);
  printf("host_meter_check OK\n");
  return 0;
}

/*
 * host_channelizer_check.cpp -- the host-only half of rdsp_channelizer_t (csrc/rdsp_channelizer_host.cpp) as a program of its
 * own, built plain and with -fsanitize=address,undefined: rdsp_channelizer_rate, _taps, _twiddles and _place on exactly sized
 * heap buffers, and their refusals.  For every configuration on the command line (P Q M D2) it prints what
 * tests/test_channelizer.py compares with the numpy restatement: the rate, a hash of the taps' bits, the twiddles' bits and
 * three placements.  Prints "host_channelizer_check OK".
 */
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "rdsp.h"

static char g_err[512];
extern "C" void rdsp_set_error(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
}
extern "C" const char *rdsp_last_error(void) { return g_err; }

static int fails = 0;
#define CHECK(c) do { if (!(c)) { printf("FAIL line %d: %s (%s)\n", __LINE__, #c, g_err); fails++; } } while (0)

static uint64_t fnv(const void *p, size_t n) {
  uint64_t h = 1469598103934665603ull;
  for (size_t i = 0; i < n; i++) h = (h ^ ((const unsigned char *)p)[i]) * 1099511628211ull;
  return h;
}

static void config(int P, int Q, int M, int D2) {
  int P1 = 0, Q1 = 0;
  CHECK(rdsp_channelizer_rate(P, Q, D2, &P1, &Q1) == RDSP_OK);
  const size_t n = (size_t)16 * (size_t)((P1 + Q1 - 1) / Q1) * (size_t)Q1;
  float *h = (float *)malloc(n * sizeof(float));
  CHECK(rdsp_channelizer_taps(P, Q, D2, h) == RDSP_OK);
  for (size_t i = 0; i < n / 2; i++) CHECK(memcmp(&h[i], &h[n - 1 - i], sizeof(float)) == 0); /* symmetric bit for bit */
  printf("config %d %d %d %d rate %d %d taps %zu %016llx\n", P, Q, M, D2, P1, Q1, n, (unsigned long long)fnv(h, n * sizeof(float)));
  free(h);
  float *tw = (float *)malloc((size_t)2 * M * sizeof(float));
  CHECK(rdsp_channelizer_twiddles(M, tw) == RDSP_OK);
  printf("twiddles");
  for (int m = 0; m < 2 * M; m++) {
    uint32_t b;
    memcpy(&b, &tw[m], 4);
    printf(" %08x", b);
  }
  printf("\n");
  CHECK(tw[0] == 1.0f && tw[1] == 0.0f && tw[2 * (M / 4)] == 0.0f && tw[2 * (M / 4) + 1] == 1.0f && tw[2 * (M / 2)] == -1.0f &&
        tw[2 * (M / 2) + 1] == 0.0f && tw[2 * (3 * M / 4)] == 0.0f && tw[2 * (3 * M / 4) + 1] == -1.0f);
  free(tw);
  const double fs = ((double)P * 44100.0) / (double)Q, spacing = fs / (double)M;
  const double st[3] = {spacing / 2.0, -spacing / 2.0, -(fs / 2.0 - 1.0)};
  for (int i = 0; i < 3; i++) {
    int k = -1;
    double res = 0.0;
    CHECK(rdsp_channelizer_place(P, Q, M, st[i], &k, &res) == RDSP_OK);
    CHECK(k >= 0 && k < M && fabs(res) <= spacing / 2.0);
    printf("place %a %d %a\n", st[i], k, res);
  }
  int k = 7;
  double res = 7.0;
  CHECK(rdsp_channelizer_place(P, Q, M, fs / 2.0, &k, &res) == RDSP_ERR_INVALID && k == 7 && res == 7.0);
  CHECK(rdsp_channelizer_place(P, Q, M, -fs / 2.0, &k, &res) == RDSP_ERR_INVALID);
  CHECK(rdsp_channelizer_place(P, Q, M, NAN, &k, &res) == RDSP_ERR_INVALID && k == 7 && res == 7.0);
}

int main(int argc, char **argv) {
  for (int a = 1; a + 3 < argc; a += 4) config(atoi(argv[a]), atoi(argv[a + 1]), atoi(argv[a + 2]), atoi(argv[a + 3]));
  int P1 = 5, Q1 = 5, k = 0;
  double res = 0.0;
  float one[16];
  CHECK(rdsp_channelizer_rate(10240, 441, 3, &P1, &Q1) == RDSP_ERR_INVALID && P1 == 5 && Q1 == 5); /* Q1 = 1323 */
  CHECK(rdsp_channelizer_rate(2, 1, 4, &P1, &Q1) == RDSP_ERR_INVALID);                              /* P1 < Q1 */
  CHECK(rdsp_channelizer_rate(16, 1, 1, &P1, &Q1) == RDSP_ERR_INVALID && rdsp_channelizer_rate(16, 1, 65, &P1, &Q1) == RDSP_ERR_INVALID);
  CHECK(rdsp_channelizer_rate(65, 1, 2, &P1, &Q1) == RDSP_ERR_INVALID && rdsp_channelizer_rate(0, 1, 2, &P1, &Q1) == RDSP_ERR_INVALID);
  CHECK(rdsp_channelizer_rate(16, 1, 4, NULL, &Q1) == RDSP_ERR_INVALID && g_err[0] != 0);
  CHECK(rdsp_channelizer_rate(32, 2, 4, &P1, &Q1) == RDSP_OK && P1 == 4 && Q1 == 1);                /* reduced first */
  CHECK(rdsp_channelizer_taps(10240, 441, 3, one) == RDSP_ERR_INVALID && rdsp_channelizer_taps(16, 1, 4, NULL) == RDSP_ERR_INVALID);
  CHECK(rdsp_channelizer_twiddles(12, one) == RDSP_ERR_INVALID && rdsp_channelizer_twiddles(8, NULL) == RDSP_ERR_INVALID);
  CHECK(rdsp_channelizer_twiddles(8, one) == RDSP_OK); /* exactly 16 floats */
  CHECK(rdsp_channelizer_place(16, 1, 12, 0.0, &k, &res) == RDSP_ERR_INVALID && rdsp_channelizer_place(65, 1, 16, 0.0, &k, &res) == RDSP_ERR_INVALID);
  CHECK(rdsp_channelizer_place(16, 1, 16, 0.0, NULL, &res) == RDSP_ERR_INVALID);
  if (fails) return 1;
  printf("host_channelizer_check OK\n");
  return 0;
}

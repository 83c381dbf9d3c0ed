/*
 * host_survey_check.c -- the host-only half of rdsp_survey_t (csrc/rdsp_survey_host.c) as a program of its own for a build with
 * -fsanitize=address,undefined: rdsp_survey_window, rdsp_survey_rows_between, rdsp_survey_bin_hz and rdsp_survey_find_stations
 * on exactly sized heap buffers, and their refusals.  Prints "host_survey_check OK".
 */
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "rdsp.h"

static char g_err[512];
void rdsp_set_error(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
}
const char *rdsp_last_error(void) { return g_err; }

static int fails = 0;
#define CHECK(c) do { if (!(c)) { printf("FAIL line %d: %s (%s)\n", __LINE__, #c, g_err); fails++; } } while (0)

static uint64_t rows_of(uint64_t n, uint64_t navg, uint64_t t) { return t < n ? 0u : ((t - n) / (n / 2u) + 1u) / navg; }

static void check_window(int n) {
  float *w = (float *)malloc((size_t)n * sizeof(float));
  CHECK(rdsp_survey_window(n, w) == RDSP_OK);
  double sum = 0.0;
  for (int i = 0; i < n; i++) sum += (double)w[i];
  CHECK(fabs(sum - 1.0) <= 1.0 / 1048576.0);
  for (int i = 1; i < n / 2; i++) /* periodic: symmetric about n / 2 (to the rounding of the two cosines), rising to it */
    CHECK(fabsf(w[i] - w[n - i]) <= 1e-6f * w[i] && w[i] > w[i - 1]);
  CHECK(w[0] > 0.0f && w[0] < 1e-6f);
  free(w);
}

/* a row with peaks at the given bins over a floor of 1.0 (with a ripple, so the floor has no plateau maxima above it) */
static float *row_with(int n, const int *bins, const float *pw, int count) {
  float *row = (float *)malloc((size_t)n * sizeof(float));
  for (int j = 0; j < n; j++) row[j] = 1.0f + 0.01f * (float)(j % 3);
  for (int c = 0; c < count; c++) {
    row[bins[c]] = pw[c];
    if (bins[c] > 0) row[bins[c] - 1] = pw[c] * 0.25f;
    if (bins[c] < n - 1) row[bins[c] + 1] = pw[c] * 0.25f;
  }
  return row;
}

int main(void) {
  check_window(1024);
  check_window(4096);
  float one;
  CHECK(rdsp_survey_window(2048, &one) == RDSP_ERR_INVALID);
  CHECK(rdsp_survey_window(1024, NULL) == RDSP_ERR_INVALID);

  /* the schedule: a walk of ragged calls, 0-pair calls included, from 0 and from above 2^32 */
  static const size_t steps[] = {1, 511, 0, 512, 1025, 777, 0, 4096, 3, 20000, 2047, 2048, 2049};
  static const uint64_t starts[] = {0u, 4294967296u + 12345u};
  for (int n = 1024; n <= 4096; n *= 4)
    for (int navg = 1; navg <= 256; navg *= 4)
      for (size_t s = 0; s < sizeof starts / sizeof starts[0]; s++) {
        uint64_t t = starts[s];
        for (int rep = 0; rep < 3; rep++)
          for (size_t k = 0; k < sizeof steps / sizeof steps[0]; k++) {
            const uint64_t want = rows_of((uint64_t)n, (uint64_t)navg, t + steps[k]) - rows_of((uint64_t)n, (uint64_t)navg, t);
            CHECK((uint64_t)rdsp_survey_rows_between(n, navg, t, steps[k]) == want);
            t += steps[k];
          }
      }
  CHECK(rdsp_survey_rows_between(1024, 1, 0, 1023) == 0 && rdsp_survey_rows_between(1024, 1, 0, 1024) == 1);
  CHECK(rdsp_survey_rows_between(1024, 1, 1024, 511) == 0 && rdsp_survey_rows_between(1024, 1, 1024, 512) == 1);
  CHECK(rdsp_survey_rows_between(512, 4, 0, 10) == RDSP_ERR_INVALID);
  CHECK(rdsp_survey_rows_between(1024, 3, 0, 10) == RDSP_ERR_INVALID);
  CHECK(rdsp_survey_rows_between(1024, 512, 0, 10) == RDSP_ERR_INVALID);
  CHECK(rdsp_survey_rows_between(1024, 0, 0, 10) == RDSP_ERR_INVALID);

  /* the axis */
  CHECK(rdsp_survey_bin_hz(1024, 160, 147, 512) == 0.0);
  CHECK(fabs(rdsp_survey_bin_hz(1024, 160, 147, 513) - 46.875) < 1e-9);
  CHECK(fabs(rdsp_survey_bin_hz(4096, 8000, 147, 0) + 1200000.0) < 1e-6);

  /* the finder on exactly sized buffers */
  for (int n = 1024; n <= 4096; n *= 4) {
    const int bins[4] = {0, n - 1, n / 2 + 100, n / 4};
    const float pw[4] = {1e6f, 1e6f, 1e4f, 1e5f};
    float *row = row_with(n, bins, pw, 4);
    double *hz = (double *)malloc(2 * sizeof(double));
    float *p = (float *)malloc(2 * sizeof(float));
    /* bins 0 and n - 1 are never reported, whatever they hold */
    int got = rdsp_survey_find_stations(row, n, 1, 1, 20.0, 0.0, 2, hz, p);
    CHECK(got == 2);
    CHECK(got == 2 && hz[0] == rdsp_survey_bin_hz(n, 1, 1, n / 4) && p[0] == 1e5f);
    CHECK(got == 2 && hz[1] == rdsp_survey_bin_hz(n, 1, 1, n / 2 + 100) && p[1] == 1e4f);
    /* max_out below the count: the strongest; no power wanted; nothing wanted */
    got = rdsp_survey_find_stations(row, n, 1, 1, 20.0, 0.0, 1, hz, NULL);
    CHECK(got == 1 && hz[0] == rdsp_survey_bin_hz(n, 1, 1, n / 4));
    CHECK(rdsp_survey_find_stations(row, n, 1, 1, 20.0, 0.0, 0, NULL, NULL) == 0);
    /* a spacing wider than the band keeps the strongest only */
    CHECK(rdsp_survey_find_stations(row, n, 1, 1, 20.0, 1e9, 2, hz, p) == 1);
    /* a threshold above every peak */
    CHECK(rdsp_survey_find_stations(row, n, 1, 1, 70.0, 0.0, 2, hz, p) == 0);
    /* an asymmetric peak is placed towards its stronger neighbour, within half a bin */
    row[n / 4 + 1] = 0.9e5f;
    got = rdsp_survey_find_stations(row, n, 1, 1, 20.0, 1e9, 2, hz, p);
    CHECK(got == 1 && hz[0] > rdsp_survey_bin_hz(n, 1, 1, n / 4) && hz[0] <= rdsp_survey_bin_hz(n, 1, 1, n / 4) + 0.5 * 44100.0 / n);
    /* a flat row, zeros, NaN and inf: nothing, or something finite, never a fault */
    for (int j = 0; j < n; j++) row[j] = 3.0f;
    CHECK(rdsp_survey_find_stations(row, n, 1, 1, 20.0, 0.0, 2, hz, p) == 0);
    memset(row, 0, (size_t)n * sizeof(float));
    CHECK(rdsp_survey_find_stations(row, n, 1, 1, 20.0, 0.0, 2, hz, p) == 0);
    row[5] = NAN;
    row[9] = INFINITY;
    got = rdsp_survey_find_stations(row, n, 1, 1, 20.0, 0.0, 2, hz, p);
    CHECK(got == 1 && hz[0] == rdsp_survey_bin_hz(n, 1, 1, 9));
    /* refusals */
    CHECK(rdsp_survey_find_stations(NULL, n, 1, 1, 20.0, 0.0, 2, hz, p) == RDSP_ERR_INVALID);
    CHECK(rdsp_survey_find_stations(row, n / 2, 1, 1, 20.0, 0.0, 2, hz, p) == RDSP_ERR_INVALID);
    CHECK(rdsp_survey_find_stations(row, n, 0, 1, 20.0, 0.0, 2, hz, p) == RDSP_ERR_INVALID);
    CHECK(rdsp_survey_find_stations(row, n, 1, 1, 20.0, -1.0, 2, hz, p) == RDSP_ERR_INVALID);
    CHECK(rdsp_survey_find_stations(row, n, 1, 1, 20.0, 0.0, -1, hz, p) == RDSP_ERR_INVALID);
    CHECK(rdsp_survey_find_stations(row, n, 1, 1, 20.0, 0.0, 2, NULL, p) == RDSP_ERR_INVALID);
    free(row); free(hz); free(p);
  }
  if (fails) return 1;
  printf("host_survey_check OK\n");
  return 0;
}

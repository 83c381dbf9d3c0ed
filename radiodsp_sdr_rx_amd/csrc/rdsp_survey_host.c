/*
 * rdsp_survey_host.c -- the host-only half of rdsp_survey_t (include/rdsp.h): the window, the row schedule, the frequency
 * axis and the station finder.  Plain C, no device: the object (rdsp_survey.hip) calls the first two, and
 * tests/host/host_survey_check.c links this file alone.
 */
#include <math.h>
#include <stdlib.h>

#include "rdsp_host.h"

static int survey_fft_ok(int fft_n) { return fft_n == 1024 || fft_n == 4096; }

/* the periodic 4-term Blackman-Harris window in double, divided by its double sum (taken in tap order), rounded to float */
int rdsp_survey_window(int fft_n, float *out) {
  if (!survey_fft_ok(fft_n) || !out) {
    rdsp_set_error("rdsp_survey_window: fft_n is 1024 or 4096, out not NULL");
    return RDSP_ERR_INVALID;
  }
  double *w = (double *)malloc((size_t)fft_n * sizeof(double)), sum = 0.0;
  if (!w) {
    rdsp_set_error("rdsp_survey_window: out of memory");
    return RDSP_ERR_NOMEM;
  }
  for (int n = 0; n < fft_n; n++) {
    const double a = 2.0 * 3.14159265358979323846 * (double)n / (double)fft_n;
    w[n] = 0.35875 - 0.48829 * cos(a) + 0.14128 * cos(2.0 * a) - 0.01168 * cos(3.0 * a);
    sum += w[n];
  }
  for (int n = 0; n < fft_n; n++) out[n] = (float)(w[n] / sum);
  free(w);
  return RDSP_OK;
}

static uint64_t survey_rows(uint64_t n, uint64_t h, uint64_t navg, uint64_t t) { return t < n ? 0u : ((t - n) / h + 1u) / navg; }

static int survey_navg_ok(int navg) { return navg >= 1 && navg <= 256 && (navg & (navg - 1)) == 0; }

/* rows(T + pairs) - rows(T), rows(T) = T < N ? 0 : ((T - N) / H + 1) / navg */
int rdsp_survey_rows_between(int fft_n, int navg, uint64_t pairs_before, size_t pairs) {
  if (!survey_fft_ok(fft_n) || !survey_navg_ok(navg)) {
    rdsp_set_error("rdsp_survey_rows_between: fft_n is 1024 or 4096, navg a power of two 1 ... 256");
    return RDSP_ERR_INVALID;
  }
  const uint64_t n = (uint64_t)fft_n, h = n / 2u, a = (uint64_t)navg;
  const uint64_t r = survey_rows(n, h, a, pairs_before + (uint64_t)pairs) - survey_rows(n, h, a, pairs_before);
  if (r > 0x7fffffffu) {
    rdsp_set_error("rdsp_survey_rows_between: %llu rows do not fit the result", (unsigned long long)r);
    return RDSP_ERR_INVALID;
  }
  return (int)r;
}

/* output index j of a row is (j - N / 2) fs / N Hz from the band centre, fs = 44100 P / Q */
double rdsp_survey_bin_hz(int fft_n, int P, int Q, int j) {
  return ((double)(j - fft_n / 2) * 44100.0 * (double)P) / ((double)Q * (double)fft_n);
}

typedef struct { int j; float p; } survey_cand_t;
static int survey_cand_cmp(const void *a, const void *b) { /* descending power, then ascending bin */
  const survey_cand_t *x = (const survey_cand_t *)a, *y = (const survey_cand_t *)b;
  if (x->p != y->p) return x->p > y->p ? -1 : 1;
  return x->j - y->j;
}
static int survey_dbl_cmp(const void *a, const void *b) {
  const double x = *(const double *)a, y = *(const double *)b;
  return x < y ? -1 : x > y;
}

int rdsp_survey_find_stations(const float *row, int fft_n, int P, int Q, double min_db_over_floor, double min_spacing_hz,
                              int max_out, double *station_hz, float *power) {
  if (!row || !survey_fft_ok(fft_n) || P < 1 || Q < 1 || max_out < 0 || (max_out > 0 && !station_hz) ||
      !(min_spacing_hz >= 0.0) || min_db_over_floor != min_db_over_floor) {
    rdsp_set_error("rdsp_survey_find_stations: bad argument");
    return RDSP_ERR_INVALID;
  }
  const int n = fft_n;
  double *db = (double *)malloc((size_t)n * sizeof(double)), *sorted = (double *)malloc((size_t)n * sizeof(double));
  survey_cand_t *cand = (survey_cand_t *)malloc((size_t)n * sizeof(survey_cand_t));
  if (!db || !sorted || !cand) {
    free(db); free(sorted); free(cand);
    rdsp_set_error("rdsp_survey_find_stations: out of memory");
    return RDSP_ERR_NOMEM;
  }
  for (int j = 0; j < n; j++) {
    const double v = (double)row[j];
    sorted[j] = db[j] = 10.0 * log10(v > 1e-30 ? v : 1e-30); /* NaN compares false: 1e-30 */
  }
  qsort(sorted, (size_t)n, sizeof(double), survey_dbl_cmp);
  const double floor_db = 0.5 * (sorted[n / 2 - 1] + sorted[n / 2]); /* the median of an even count */
  int nc = 0;
  for (int j = 1; j <= n - 2; j++)
    if (db[j] >= floor_db + min_db_over_floor && row[j] >= row[j - 1] && row[j] > row[j + 1]) {
      cand[nc].j = j;
      cand[nc++].p = row[j];
    }
  qsort(cand, (size_t)nc, sizeof(survey_cand_t), survey_cand_cmp);
  const double bin = rdsp_survey_bin_hz(fft_n, P, Q, fft_n / 2 + 1);
  int taken = 0;
  for (int c = 0; c < nc && taken < max_out; c++) {
    const int j = cand[c].j;
    /* the vertex of the parabola through the three dB values; a candidate is a local maximum, so it lies within half a bin */
    const double a = db[j - 1], b = db[j], d = db[j + 1], den = a - 2.0 * b + d;
    double off = den < 0.0 ? 0.5 * (a - d) / den : 0.0;
    off = off < -0.5 ? -0.5 : off > 0.5 ? 0.5 : off;
    const double hz = rdsp_survey_bin_hz(fft_n, P, Q, j) + off * bin;
    int k = 0;
    while (k < taken && fabs(hz - station_hz[k]) >= min_spacing_hz) k++;
    if (k < taken) continue;
    station_hz[taken] = hz;
    if (power) power[taken] = row[j];
    taken++;
  }
  free(db); free(sorted); free(cand);
  return taken;
}

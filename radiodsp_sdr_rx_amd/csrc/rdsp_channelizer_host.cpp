/*
 * rdsp_channelizer_host.cpp -- the host-only half of rdsp_channelizer_t (include/rdsp.h): the sub-band rate, the prototype, the
 * twiddle table and the placement of a station.  No device: the object (rdsp_channelizer.hip) calls the first three, and
 * tests/host/host_channelizer_check.cpp links this file alone.  The prototype and the rule for source rates are rdsp_tune.h's.
 */
#include <math.h>

#include "rdsp_channelizer.h"
#include "rdsp_host.h"

extern "C" {

int rdsp_channelizer_rate(int P, int Q, int D2, int *P1, int *Q1) {
  int p1 = 0, q1 = 0;
  if (!P1 || !Q1 || !rdsp_chan::rate(P, Q, D2, p1, q1)) {
    rdsp_set_error("rdsp_channelizer_rate: P / Q = %d / %d must pass the engine's rule for source rates, D2 = %d lie in %d ... %d, and "
                   "P1 / Q1 = P / (Q D2) in lowest terms have P1 >= Q1 and Q1 <= %d", P, Q, D2, rdsp_chan::MIN_D2, rdsp_chan::MAX_D2,
                   rdsp_tune::RATE_MAX_Q);
    return RDSP_ERR_INVALID;
  }
  *P1 = p1; *Q1 = q1;
  return RDSP_OK;
}

/* rdsp_tune::rate_taps(P1, Q1, 1.0) times 2^-15 (exact): Tb Q1 floats in the prototype's order, branch r is out[j Q1 + r] */
int rdsp_channelizer_taps(int P, int Q, int D2, float *out) {
  int P1, Q1;
  const int rc = rdsp_channelizer_rate(P, Q, D2, &P1, &Q1);
  if (rc != RDSP_OK) return rc;
  if (!out) {
    rdsp_set_error("rdsp_channelizer_taps: out is NULL");
    return RDSP_ERR_INVALID;
  }
  rdsp_tune::rate_taps(P1, Q1, 1.0, out);
  const size_t n = (size_t)rdsp_tune::rate_tb(P1, Q1) * (size_t)Q1;
  for (size_t i = 0; i < n; i++) out[i] *= 0x1p-15f;
  return RDSP_OK;
}

/* (cos, sin)(2 pi m / M): the first octant by libm in double, rounded to float; the rest by symmetry, so the table is exactly
 * 0 and +-1 at quarter turns and the same magnitudes return in every octant; no negative zero */
int rdsp_channelizer_twiddles(int M, float *out) {
  if (!rdsp_chan::m_ok(M) || !out) {
    rdsp_set_error("rdsp_channelizer_twiddles: M is 8, 16, 32 or 64, out not NULL");
    return RDSP_ERR_INVALID;
  }
  const int quarter = M / 4, eighth = M / 8;
  for (int m = 0; m < M; m++) {
    const int turn = m / quarter, rem = m % quarter;
    const int b = rem <= eighth ? rem : quarter - rem; /* the angle inside the first octant */
    const double a = 2.0 * 3.14159265358979323846 * (double)b / (double)M;
    float c = (float)cos(a), s = (float)sin(a);
    if (b == 0) { c = 1.0f; s = 0.0f; }
    if (b == eighth) s = c;
    if (rem > eighth) { const float t = c; c = s; s = t; }
    float x = c, y = s;
    if (turn == 1) { x = -s; y = c; }
    if (turn == 2) { x = -c; y = -s; }
    if (turn == 3) { x = s; y = -c; }
    out[2 * m] = x + 0.0f;
    out[2 * m + 1] = y + 0.0f;
  }
  return RDSP_OK;
}

/* all in double: kk = station / spacing rounded half away from zero; sub-band kk mod M; residual = station - kk spacing */
int rdsp_channelizer_place(int P, int Q, int M, double station_hz, int *subband, double *residual_hz) {
  if (!rdsp_tune::rate_reduce(P, Q) || !rdsp_chan::m_ok(M) || !subband || !residual_hz) {
    rdsp_set_error("rdsp_channelizer_place: P / Q must pass the engine's rule for source rates, M be 8, 16, 32 or 64");
    return RDSP_ERR_INVALID;
  }
  const double fs = ((double)P * rdsp_tune::TUNE_FS) / (double)Q;
  if (!(fabs(station_hz) < fs / 2.0)) {
    rdsp_set_error("rdsp_channelizer_place: station %g Hz; |f| must be below %g Hz", station_hz, fs / 2.0);
    return RDSP_ERR_INVALID;
  }
  const double spacing = fs / (double)M; /* exact: M is a power of two */
  const double kk = round(station_hz / spacing);
  const int k = (int)kk;
  *subband = ((k % M) + M) % M;
  *residual_hz = station_hz - kk * spacing;
  return RDSP_OK;
}

}  // extern "C"
